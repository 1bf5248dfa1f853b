"""CPU checker of the keypoint evaluator (simple_pose_amd.metrics.coco_eval): a plain, loop-by-loop numpy float64 restatement of
pycocotools' COCOeval(gt, dt, "keypoints") - loadRes, computeOks, evaluateImg, accumulate, summarize - written for reading, not for
speed, plus the seeded generator of annotation dicts and detections the tests use.  It shares no code with the package (it has its
own parameter tables) and returns every intermediate."""
import numpy as np

STAT_NAMES = ['AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']
IOU_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(0., 1., 101)
AREA_RNG = [[0., 1e10], [32. ** 2, 96. ** 2], [96. ** 2, 1e10]]          # all, medium, large
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
EPS = np.spacing(1)                                                        # 2^-52


def compute_oks(dts, gts, sigmas):
    """[len(dts), len(gts)]: detections in the given (score) order against ground truths in annotation order."""
    ious = np.zeros((len(dts), len(gts)))
    vars_ = (sigmas * 2) ** 2
    k = len(sigmas)
    for j, gt in enumerate(gts):
        g = np.array(gt['keypoints'], dtype=np.float64)
        xg, yg, vg = g[0::3], g[1::3], g[2::3]
        k1 = np.count_nonzero(vg > 0)
        bb = gt['bbox']
        x0, x1 = bb[0] - bb[2], bb[0] + bb[2] * 2
        y0, y1 = bb[1] - bb[3], bb[1] + bb[3] * 2
        for i, dt in enumerate(dts):
            d = np.array(dt['keypoints'], dtype=np.float64)
            xd, yd = d[0::3], d[1::3]
            if k1 > 0:
                dx = xd - xg
                dy = yd - yg
            else:
                z = np.zeros(k)
                dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
            e = (dx ** 2 + dy ** 2) / vars_ / (gt['area'] + EPS) / 2
            if k1 > 0:
                e = e[vg > 0]
            ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
    return ious


def evaluate_img(gts, dts, ious, area_rng, iou_thrs):
    """One image, one area range.  dts are in score order (already cut); returns dtm [T,D] (annotation id, 0 = none), dt_ignore [T,D],
    gt_ignore [G] in ANNOTATION order."""
    G, D, T = len(gts), len(dts), len(iou_thrs)
    ig = [bool(g['_base_ignore'] or g['area'] < area_rng[0] or g['area'] > area_rng[1]) for g in gts]
    order = [i for i in range(G) if not ig[i]] + [i for i in range(G) if ig[i]]          # stable, non-ignored first
    gtm = np.zeros((T, G), dtype=np.int64)
    dtm = np.zeros((T, D), dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    for tind, t in enumerate(iou_thrs):
        for dind, d in enumerate(dts):
            best = min(t, 1 - 1e-10)
            m = -1
            for g in order:
                if gtm[tind, g] > 0 and not gts[g]['_crowd']:
                    continue
                if m > -1 and not ig[m] and ig[g]:
                    break
                if ious[dind, g] < best:
                    continue
                best = ious[dind, g]
                m = g
            if m == -1:
                continue
            dt_ig[tind, dind] = ig[m]
            dtm[tind, dind] = gts[m]['id']
            gtm[tind, m] = d['id']
    for dind, d in enumerate(dts):
        outside = d['area'] < area_rng[0] or d['area'] > area_rng[1]
        for tind in range(T):
            if dtm[tind, dind] == 0 and outside:
                dt_ig[tind, dind] = True
    return dtm, dt_ig, np.array(ig, dtype=bool)


def evaluate(gt, results, sigmas=None, max_dets=20):
    """gt: dict with 'images' and 'annotations'; results: list of result dicts.  Returns a dict of every intermediate, per image id:
    'oks' [D,G], 'dt_ids' [D], 'dtm' [3,10,D], 'dt_ignore' [3,10,D], 'gt_ignore' [3,G]; and 'precision' [10,101,3], 'recall' [10,3],
    'stats' [10]."""
    sigmas = SIGMAS if sigmas is None else np.asarray(sigmas, dtype=np.float64)
    img_ids = sorted(im['id'] for im in gt['images'])
    gts = {i: [] for i in img_ids}
    dts = {i: [] for i in img_ids}
    for n, a in enumerate(gt['annotations']):
        if a['image_id'] not in gts:
            raise ValueError("annotation of an image that is not listed")
        g = dict(a)
        g.setdefault('id', n + 1)
        g['_crowd'] = bool(a.get('iscrowd', 0))
        g['_base_ignore'] = bool(a.get('ignore', 0)) or g['_crowd'] or a['num_keypoints'] == 0
        gts[a['image_id']].append(g)
    for n, r in enumerate(results):                                                    # loadRes
        if r['image_id'] not in dts:
            raise ValueError("result %d: image_id %r is not in the ground truth's images" % (n, r['image_id']))
        d = dict(r)
        d['id'] = n + 1
        kp = np.array(r['keypoints'], dtype=np.float64)
        x, y = kp[0::3], kp[1::3]
        d['area'] = (np.max(x) - np.min(x)) * (np.max(y) - np.min(y))
        dts[r['image_id']].append(d)
    T, R, A = len(IOU_THRS), len(REC_THRS), len(AREA_RNG)
    out = {'oks': {}, 'dt_ids': {}, 'dtm': {}, 'dt_ignore': {}, 'gt_ignore': {}}
    for i in img_ids:                                                                  # evaluate()
        order = sorted(range(len(dts[i])), key=lambda n: -dts[i][n]['score'])          # sorted() is stable
        dts[i] = [dts[i][n] for n in order][:max_dets]
        out['oks'][i] = compute_oks(dts[i], gts[i], sigmas)
        out['dt_ids'][i] = np.array([d['id'] for d in dts[i]], dtype=np.int64)
        per_area = [evaluate_img(gts[i], dts[i], out['oks'][i], rng, IOU_THRS) for rng in AREA_RNG]
        out['dtm'][i] = np.stack([p[0] for p in per_area]).reshape(A, T, len(dts[i]))
        out['dt_ignore'][i] = np.stack([p[1] for p in per_area]).reshape(A, T, len(dts[i]))
        out['gt_ignore'][i] = np.stack([p[2] for p in per_area]).reshape(A, len(gts[i]))
    precision = -np.ones((T, R, A))                                                    # accumulate()
    recall = -np.ones((T, A))
    for a in range(A):
        scores, dtm, dt_ig, npig = [], [], [], 0
        for i in img_ids:
            if not gts[i] and not dts[i]:
                continue
            scores += [d['score'] for d in dts[i]]
            dtm.append(out['dtm'][i][a])
            dt_ig.append(out['dt_ignore'][i][a])
            npig += int(np.count_nonzero(~out['gt_ignore'][i][a]))
        if npig == 0:
            continue
        nd = len(scores)
        inds = np.argsort(-np.array(scores, dtype=np.float64), kind='mergesort')
        dtm = np.concatenate(dtm, axis=1)[:, inds] if nd else np.zeros((T, 0), dtype=np.int64)
        dt_ig = np.concatenate(dt_ig, axis=1)[:, inds] if nd else np.zeros((T, 0), dtype=bool)
        for t in range(T):
            tp = np.zeros(nd)
            fp = np.zeros(nd)
            ntp = nfp = 0
            for n in range(nd):
                if not dt_ig[t, n]:
                    if dtm[t, n] != 0:
                        ntp += 1
                    else:
                        nfp += 1
                tp[n], fp[n] = ntp, nfp
            rc = tp / npig
            pr = tp / (fp + tp + EPS)
            recall[t, a] = rc[-1] if nd else 0
            pr = pr.tolist()
            for n in range(nd - 1, 0, -1):
                if pr[n] > pr[n - 1]:
                    pr[n - 1] = pr[n]
            q = np.zeros(R)
            for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side='left')):
                if pi < nd:
                    q[ri] = pr[pi]
            precision[t, :, a] = q
    out['precision'], out['recall'] = precision, recall
    out['stats'] = summarize(precision, recall)
    return out


def summarize(precision, recall):
    def one(ap, thr, a):
        s = precision[:, :, a] if ap else recall[:, a]
        if thr is not None:
            s = s[np.where(thr == IOU_THRS)[0]]
        s = s[s > -1]
        return np.mean(s) if len(s) else -1.0
    return np.array([one(1, None, 0), one(1, .5, 0), one(1, .75, 0), one(1, None, 1), one(1, None, 2),
                     one(0, None, 0), one(0, .5, 0), one(0, .75, 0), one(0, None, 1), one(0, None, 2)])


def threshold_margin(oks_by_image):
    """Smallest distance of any OKS value to any of the ten thresholds or to 1 - 1e-10 (inf without values)."""
    marks = np.concatenate([IOU_THRS, [1 - 1e-10]])
    vals = np.concatenate([o.reshape(-1) for o in oks_by_image.values()] + [np.zeros(0)])
    return float(np.abs(vals[:, None] - marks[None, :]).min()) if vals.size else float('inf')


# ---- seeded data ----------------------------------------------------------------------------------------------------------------------------
def person(rng, x, y, w, h, vis_prob=0.8):
    """17 key points inside the box (x, y, w, h): [17,3] with v in {0,1,2}; invisible joints are (0,0,0) as in COCO."""
    k = np.zeros((17, 3))
    k[:, 0] = np.round(x + rng.uniform(0.05, 0.95, 17) * w)
    k[:, 1] = np.round(y + rng.uniform(0.05, 0.95, 17) * h)
    k[:, 2] = np.where(rng.uniform(size=17) < vis_prob, rng.integers(1, 3, 17), 0)
    k[k[:, 2] == 0] = 0
    return k


def annotation(ann_id, image_id, kps, box, area, iscrowd=0, num_keypoints=None):
    return {'id': ann_id, 'image_id': image_id, 'category_id': 1, 'keypoints': [float(v) for v in kps.reshape(-1)],
            'num_keypoints': int((kps[:, 2] > 0).sum()) if num_keypoints is None else num_keypoints,
            'bbox': [float(v) for v in box], 'area': float(area), 'iscrowd': iscrowd}


def result(image_id, xy, maxvals, score):
    """A result dict as kps_to_dict_ writes it: fp32 values widened to Python floats."""
    k = np.concatenate([np.asarray(xy, np.float32), np.asarray(maxvals, np.float32).reshape(-1, 1)], axis=1)
    return {'image_id': image_id, 'score': float(np.float32(score)), 'category_id': 1, 'keypoints': [float(v) for v in k.reshape(-1)]}


def make_dataset(seed, n_images=300, crowded_every=11, width=640, height=480, max_gt=4, crowded_copies=(6, 12)):
    """A seeded annotation dict + result list that holds every situation at once: small / medium / large persons, crowd and
    zero-keypoint ground truths, images with ground truths and no detections and the reverse, empty images, images with more than 20
    detections, tied scores (a two-decimal grid), detection noise at several scales.  Returns (gt dict, results, arrays) where arrays =
    (xy float32 [P,17,2], maxvals float32 [P,17], scores float32 [P], image ids [P]) are the results as decoder output."""
    rng = np.random.default_rng(seed)
    ids = [int(v) for v in rng.permutation(np.arange(1000, 1000 + 3 * n_images))[:n_images]]
    anns, xy, mv, sc, im = [], [], [], [], []
    for n, image_id in enumerate(ids):
        kind = n % 10                                           # 7: ground truths only, 8: detections only, 9: empty image
        n_gt = 0 if kind in (8, 9) else int(rng.integers(1, max_gt + 1))
        mine = []
        for _ in range(n_gt):
            cls = rng.integers(0, 3)                            # small, medium, large
            h = float([rng.uniform(14, 34), rng.uniform(45, 110), rng.uniform(130, 400)][cls])
            w = h * float(rng.uniform(0.35, 0.7))
            x, y = float(rng.uniform(0, width - w)), float(rng.uniform(0, height * 0.9))
            k = person(rng, x, y, w, h)
            special = rng.uniform()
            if special < 0.08:                                  # a person without labelled key points: a small box, ignored
                w, h = float(rng.uniform(3, 8)), float(rng.uniform(3, 8))
                k = np.zeros((17, 3))
                a = annotation(len(anns) + 1, image_id, k, (x, y, w, h), 0.7 * w * h)
            elif special < 0.18:                                # a crowd region
                a = annotation(len(anns) + 1, image_id, k, (x, y, w, h), 0.7 * w * h, iscrowd=1)
            else:
                a = annotation(len(anns) + 1, image_id, k, (x, y, w, h), 0.7 * w * h)
            anns.append(a)
            mine.append((a, k, (x, y, w, h)))
        if kind == 7:
            continue
        crowded = n % crowded_every == 0
        for a, k, (x, y, w, h) in mine:                         # noisy copies of the ground truths
            copies = int(rng.integers(*crowded_copies)) if crowded or a['iscrowd'] else int(rng.integers(0, 3))
            if a['num_keypoints'] == 0:
                copies = 0                                      # (a detection inside its doubled box would have OKS exactly 1)
            for _ in range(copies):
                noise = float(rng.choice([0.03, 0.06, 0.12, 0.25])) * np.sqrt(a['area'])
                p = k[:, :2] + rng.normal(0, 1, (17, 2)) * noise
                hidden = k[:, 2] == 0
                p[hidden] = np.stack([x + rng.uniform(0, 1, 17) * w, y + rng.uniform(0, 1, 17) * h], 1)[hidden]
                xy.append(p); im.append(image_id)
        for _ in range(int(rng.integers(1, 4)) if kind == 8 or rng.uniform() < 0.4 else 0):      # unrelated detections
            h = float(rng.uniform(20, 300))
            xy.append(person(rng, float(rng.uniform(0, width)), float(rng.uniform(0, height)), h * 0.5, h)[:, :2] + rng.uniform(0, 1, (17, 2)))
            im.append(image_id)
    P = len(xy)
    order = rng.permutation(P)                                  # results are not grouped by image
    xy = np.asarray(xy, np.float32)[order]
    im = [im[i] for i in order]
    sc = (np.round(rng.uniform(0.05, 1.0, P), 2)).astype(np.float32)
    mv = rng.uniform(0.1, 1.0, (P, 17)).astype(np.float32)
    gt = {'images': [{'id': i, 'width': width, 'height': height} for i in ids], 'annotations': anns,
          'categories': [{'id': 1, 'name': 'person'}]}
    results = [result(im[i], xy[i], mv[i], sc[i]) for i in range(P)]
    return gt, results, (xy, mv, sc, im)
