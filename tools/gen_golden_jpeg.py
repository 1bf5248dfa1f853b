"""tools/gen_golden_jpeg.py - TEST INFRASTRUCTURE.  Needs PIL (libjpeg-turbo); run where it is installed:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_jpeg.py [--check]

g15_jpeg.npz: small baseline JPEG files written by PIL and PIL's own decode of each as BGR - the pixels the device decoder has to
reproduce bit for bit.  uint8 / int32 arrays only (allow_pickle=False):

    names     uint8   the case names, newline separated
    bytes     uint8   every file, concatenated;        offsets       int32 [n+1]
    pixels    uint8   every decoded image [H,W,3] BGR; pixel_offsets int32 [n+1], shapes int32 [n,2] (H, W; 0,0 for a rejection case)
    code      int32   [n]  0 = decodable, otherwise the SP_JPEG_E* code sp_jpeg_parse has to return

Images are seeded gradients plus noise.  The cases are the smallest that reach each branch of the decoder (single MCU, odd chroma sizes,
restart intervals in rows and in MCUs, custom tables with codes longer than the lookahead, 16-bit-range coefficients, grayscale, extra
header segments, planes too narrow for the fancy filter).  A 40x40 4:2:0 image has 9 MCUs, so its one-MCU restart interval gives 9
segments; r1_72x64_444 is the file with more than 64 segments (9 x 8 = 72 MCUs), the one in which a lane of the entropy kernel takes
a second segment.
"""
from __future__ import annotations

import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g15_jpeg.npz")
SEED = 15

# name, (W, H), mode, PIL save options
CASES = [
    ("s_1x1_420", (1, 1), "RGB", dict(quality=90, subsampling=2)),
    ("s_8x8_420", (8, 8), "RGB", dict(quality=90, subsampling=2)),
    ("s_16x16_420", (16, 16), "RGB", dict(quality=90, subsampling=2)),
    ("rr_17x16_422", (17, 16), "RGB", dict(quality=85, subsampling=1, restart_marker_rows=1)),
    ("rb2_33x17_420", (33, 17), "RGB", dict(quality=85, subsampling=2, restart_marker_blocks=2)),
    ("m_37x53_444", (37, 53), "RGB", dict(quality=80, subsampling=0)),
    ("m_37x53_422", (37, 53), "RGB", dict(quality=80, subsampling=1)),
    ("m_37x53_420", (37, 53), "RGB", dict(quality=80, subsampling=2)),
    ("opt_48x64_420", (48, 64), "RGB", dict(quality=95, subsampling=2, optimize=True)),
    ("r1_40x40_420", (40, 40), "RGB", dict(quality=75, subsampling=2, restart_marker_blocks=1)),
    ("r1_72x64_444", (72, 64), "RGB", dict(quality=50, subsampling=0, restart_marker_blocks=1)),
    ("q100_24x24_420", (24, 24), "RGB", dict(quality=100, subsampling=2)),
    ("q30_20x12_422", (20, 12), "RGB", dict(quality=30, subsampling=1)),
    ("gray_40x24", (40, 24), "L", dict(quality=90)),
    ("app1_com_16x8_420", (16, 8), "RGB", dict(quality=90, subsampling=2)),
    ("n_2x2_420", (2, 2), "RGB", dict(quality=90, subsampling=2)),
    ("n_3x5_420", (3, 5), "RGB", dict(quality=90, subsampling=2)),
    ("n_4x3_422", (4, 3), "RGB", dict(quality=90, subsampling=1)),
    ("n_5x2_420", (5, 2), "RGB", dict(quality=90, subsampling=2)),
]
REJECT = [("x_progressive", jpeg_ref.E_PROGRESSIVE), ("x_precision12", jpeg_ref.E_PRECISION), ("x_4components", jpeg_ref.E_COMPONENTS),
          ("x_no_dht", jpeg_ref.E_NO_TABLE)]


def image(rng, w, h, mode):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = []
    for c in range(3 if mode == "RGB" else 1):
        a, b, p = rng.uniform(-3, 3, 3)
        g = 128 + a * (xx - w / 2) * 6 / max(w, 8) * 8 + b * (yy - h / 2) * 6 / max(h, 8) * 8 + 40 * np.sin(p + xx * 0.9 + yy * 0.6)
        ch.append(g + rng.normal(0, 12, (h, w)))
    arr = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    return arr if mode == "RGB" else arr[:, :, 0]


def find_marker(data, marker):
    """Offset of the first FF `marker` among the header segments."""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        if data[pos + 1] == marker:
            return pos
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    raise ValueError(f"no marker {marker:02X}")


def pil_bgr(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def build():
    from PIL import Image
    rng = np.random.RandomState(SEED)
    files, pix, codes, names = [], [], [], []
    for name, (w, h), mode, opts in CASES:
        buf = io.BytesIO()
        Image.fromarray(image(rng, w, h, mode), mode).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        if name.startswith("app1_com"):
            exif = b"Exif\0\0" + bytes(range(40))
            com = b"simple_pose_amd fixture"
            data = (data[:2] + b"\xff\xe1" + (len(exif) + 2).to_bytes(2, "big") + exif + b"\xff\xfe" + (len(com) + 2).to_bytes(2, "big") + com
                    + data[2:])
        files.append(data)
        names.append(name)
        pix.append(pil_bgr(data))
        codes.append(0)
    base = io.BytesIO()
    src = image(rng, 16, 16, "RGB")
    Image.fromarray(src, "RGB").save(base, "JPEG", quality=90, subsampling=2)
    base = bytearray(base.getvalue())
    prog = io.BytesIO()
    Image.fromarray(src, "RGB").save(prog, "JPEG", quality=90, subsampling=2, progressive=True)
    sof, sos = find_marker(base, 0xC0), find_marker(base, 0xDA)
    p12, c4, nodht = bytearray(base), bytearray(base), bytearray(base)
    p12[sof + 4] = 12                # sample precision
    c4[sof + 9] = 4                  # number of components
    nodht[sos + 6] = 0x22            # first scan component: DC / AC table 2, which no DHT defines
    for (name, code), data in zip(REJECT, (prog.getvalue(), bytes(p12), bytes(c4), bytes(nodht))):
        files.append(bytes(data))
        names.append(name)
        pix.append(np.zeros((0, 0, 3), np.uint8))
        codes.append(code)
    return {
        "names": np.frombuffer("\n".join(names).encode(), np.uint8),
        "bytes": np.frombuffer(b"".join(files), np.uint8),
        "offsets": np.cumsum([0] + [len(f) for f in files]).astype(np.int32),
        "pixels": np.concatenate([p.reshape(-1) for p in pix]),
        "pixel_offsets": np.cumsum([0] + [p.size for p in pix]).astype(np.int32),
        "shapes": np.array([p.shape[:2] for p in pix], np.int32),
        "code": np.array(codes, np.int32),
    }


def main():
    new = build()
    if "--check" in sys.argv:
        old = np.load(OUT, allow_pickle=False)
        bad = [k for k in new if not np.array_equal(old[k], new[k])]
        print("g15_jpeg.npz:", "identical" if not bad else f"DIFFERS in {bad}")
        return 1 if bad else 0
    np.savez_compressed(OUT, **new)
    print(f"wrote {OUT}: {len(new['offsets']) - 1} files, {new['bytes'].size} file bytes, {os.path.getsize(OUT)} bytes on disk")
    return 0


if __name__ == "__main__":
    sys.exit(main())
