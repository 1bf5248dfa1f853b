"""Persons across video frames: persistent identities on top of `TopDownPoseEstimator`, and frames that leave the detector out.

    trk = PoseTracker(estimator, slots=None, match_thre=0.5, max_age=30, detect_every=1, box_expand=1.25, sigmas=None, smooth=None)
    res = trk.update(img)      # PoseResult with track_id: int32 [n], aligned with keypoints / score / box
    trk.reset()
    trk = PoseTracker(estimator, smooth=OneEuro(min_cutoff=1.0, beta=0.5, d_cutoff=1.0, max_gap=0.5, fps=30.0))
    res = trk.update(img, timestamp=t)     # ... and keypoints_smooth: float64 [n, J, 3], the tracked poses through a One-Euro filter

The association runs on the device, on the estimator's stream, right after sp_oks_nms: sp_track_associate_images matches the frame's kept poses
with the tracks by OKS (the similarity OKS-NMS uses, the same device function), greedily, best pair first; unmatched poses start new
tracks (ids 1, 2, ... never reused), tracks unseen for more than `max_age` frames are freed.  The track state is device memory owned by
the tracker; the ids come back in the frame's packed buffer, so a tracked frame still ends in ONE device-to-host copy, and with
`estimator.use_graph` it is ONE graph replay.  There is no CPU fallback.  An estimator built with a `renderer` also draws the frame
(`PoseResult.image`, the persons coloured by track id), inside the same replay; one built with a `redactor` hides the heads or the
persons in that image first (sp_redact_u8c3, from the frame's raw key points), on detector and propagated frames alike.

Two kinds of frame, chosen by the host alone (from its own counters and the previous result, no extra synchronisation):
  detector frame    _detect -> _poses -> sp_track_associate_images: the first frame, the first after reset(), every `detect_every`-th frame (counted
                    from the last detector frame), and whenever the previous frame returned no person;
  propagated frame  sp_track_boxes_images -> _poses -> sp_track_associate_images: every other frame.  The boxes are derived from the poses the tracker
                    just saw (the tracks with miss == 0); the detector program is NOT launched at all, so persons who enter the scene
                    are only seen at the next detector frame.
Tracks live in source-image pixels: call reset() when the stream (or its size) changes; propagated boxes are clipped to the image they
are used on.

`match_thre`, `max_age` and `box_expand` are design choices, not tuned values: there are no trained weights in this repository to tune
them on.

Smoothing (`smooth=OneEuro(...)`, off by default): the poses are decoded frame by frame, so sub-pixel decode noise and the crop changing
between detector and propagated frames make a standing person's skeleton shiver.  sp_track_smooth_images, one more launch right
after the association, runs the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012: a low-pass whose cut-off rises with the speed, so slow
motion is steadied and fast motion is not lagged) per track and joint on the frame's kept poses; its state lives in device memory next to
the tracks', keyed by slot, and a slot handed to another id starts again.  The frame's time is one double in device memory that the host
writes before the launch or the replay, through a pinned buffer and a copy on the frame's stream (never a kernel argument: a captured graph
freezes those), `timestamp` in seconds or, without one, frame index / fps.  The smoothed poses come back in the same packed buffer (`PoseResult.keypoints_smooth`; the confidences are not filtered)
and are what the estimator's `renderer` draws, inside the same replay (its `redactor` keeps reading the raw poses: the face is where this
frame's decode put it, not where the filter lags to).  `keypoints`, `score`, `box`, `track_id`, the association and the
propagated boxes keep using the raw poses: they are bit for bit what they are without smoothing.  Speeds are measured in body sizes (the
box's longer side) per second, so the parameters do not depend on the resolution.  OneEuro's defaults are design choices as well.

ONE implementation: `MultiStreamTracker(estimator, streams=S, ...)` tracks S same-sized video streams in ONE call - one frame of batch S,
the sp_track_*_images entries on stream-major state, one frame kind per call, every stream's result bit for bit what a tracker of its own
returns (see the class).  It owns the state, the launches, the graph cache and the frame-kind rule.  `PoseTracker` is its one-stream face:
a subclass with streams=1 that takes one image, returns one PoseResult and shows `state` / `smooth_state` without the stream axis, as views
of the same memory.  The library's single-image entries (sp_track_associate, sp_track_boxes, sp_track_smooth) are images = 1 calls of the
same device code and are not called from here."""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from . import _lib
from .pipeline import PoseResult, TopDownPoseEstimator, _Frame, capture_graph

P = _lib.ptr
MAX_SLOTS = 256                      # one thread per track in the match kernel (sp_track_associate)


def _positive(name, v, what, zero_ok=False):
    if not isinstance(v, (int, float)) or isinstance(v, bool) or not ((0.0 <= float(v) if zero_ok else 0.0 < float(v)) and float(v) < float("inf")):
        raise ValueError(f"{name}: {what}, got {v!r}")
    return float(v)


class OneEuro(object):
    """The parameters of the tracker's key-point smoother (sp_track_smooth).  `min_cutoff`: the cut-off frequency at rest, Hz (> 0; lower is
    steadier and lags more).  `beta`: how fast the cut-off rises with the speed, per body size per second (>= 0; 0 is a fixed low-pass).
    `d_cutoff`: the cut-off of the speed estimate, Hz (> 0).  `max_gap`: seconds without an accepted sample after which a joint starts again
    from the raw value (> 0).  `fps`: the frame rate `update` assumes when it gets no timestamp (> 0).  The defaults are design choices, not
    tuned values: there are no trained weights and no video in this repository to tune them on."""

    def __init__(self, min_cutoff: float = 1.0, beta: float = 0.5, d_cutoff: float = 1.0, max_gap: float = 0.5, fps: float = 30.0):
        self.min_cutoff = _positive("min_cutoff", min_cutoff, "a frequency > 0 (Hz)")
        self.beta = _positive("beta", beta, "a finite factor >= 0", zero_ok=True)
        self.d_cutoff = _positive("d_cutoff", d_cutoff, "a frequency > 0 (Hz)")
        self.max_gap = _positive("max_gap", max_gap, "a time > 0 (seconds)")
        self.fps = _positive("fps", fps, "a frame rate > 0")

    def key(self) -> tuple:
        """Everything sp_track_smooth's launch depends on (a captured graph is reused only while it is unchanged)."""
        return (self.min_cutoff, self.beta, self.d_cutoff, self.max_gap)

    def __repr__(self) -> str:
        return f"OneEuro(min_cutoff={self.min_cutoff}, beta={self.beta}, d_cutoff={self.d_cutoff}, max_gap={self.max_gap}, fps={self.fps})"


def _tracker_args(estimator, slots, match_thre, max_age, detect_every, box_expand, sigmas, smooth):
    """What PoseTracker and MultiStreamTracker refuse at construction -> (slots, sigmas) as they are kept."""
    if not isinstance(estimator, TopDownPoseEstimator):
        raise TypeError(f"estimator: expected a TopDownPoseEstimator, got {type(estimator).__name__}")
    if slots is None:
        slots = estimator.capacity
    if not isinstance(slots, int) or isinstance(slots, bool) or slots < 1:
        raise ValueError(f"slots: expected an int in 1..{MAX_SLOTS}, got {slots!r}")
    if slots > MAX_SLOTS:
        raise ValueError(f"slots: {slots} exceeds the tracker's limit of {MAX_SLOTS} tracks (one thread per track in the match kernel); "
                         f"use an estimator with capacity <= {MAX_SLOTS} or pass slots explicitly")
    if slots < estimator.capacity:
        raise ValueError(f"slots: {slots} is below the estimator's capacity {estimator.capacity}; every person of a frame needs a slot")
    if not isinstance(match_thre, (int, float)) or isinstance(match_thre, bool) or not (0.0 < float(match_thre) <= 1.0):
        raise ValueError(f"match_thre: an OKS in (0, 1], got {match_thre!r}")
    if not isinstance(max_age, int) or isinstance(max_age, bool) or max_age < 0:
        raise ValueError(f"max_age: a frame count >= 0, got {max_age!r}")
    if not isinstance(detect_every, int) or isinstance(detect_every, bool) or detect_every < 1:
        raise ValueError(f"detect_every: an int >= 1, got {detect_every!r}")
    if not isinstance(box_expand, (int, float)) or isinstance(box_expand, bool) or not (0.0 < float(box_expand) < float("inf")):
        raise ValueError(f"box_expand: a positive factor, got {box_expand!r}")
    if sigmas is not None:
        sigmas = np.asarray(sigmas, np.float64).reshape(-1)
        if sigmas.size < 1 or sigmas.size > 64 or not (np.isfinite(sigmas).all() and (sigmas > 0).all()):
            raise ValueError("sigmas: expected 1..64 positive per-joint values")
    if smooth is not None and not isinstance(smooth, OneEuro):
        raise TypeError(f"smooth: expected a simple_pose_amd.tracking.OneEuro or None, got {type(smooth).__name__}")
    return slots, sigmas


MAX_STREAMS = 256                    # sp_track_*_images: `images` 1 .. 256


class MultiStreamTracker(object):
    """S video streams tracked in ONE call: one detector forward on the S frames (or sp_track_boxes_images in its place), one pose forward
    on the estimator's `capacity` crops, sp_track_associate_images, sp_track_smooth_images, the overlay, and one device-to-host copy - a
    launch count that does not grow with S, and with `estimator.use_graph` one graph replay.  Every stream's result is bit for bit what a
    tracker of its own returns for the same frames under the same frame kinds: the state is stream-major (`state[k][s]` is stream s's,
    ids start at 1 in every stream) and no stream reads another's.

        trk = MultiStreamTracker(estimator, streams=S, slots=None, match_thre=0.5, max_age=30, detect_every=1, box_expand=1.25,
                                 sigmas=None, smooth=None)
        results = trk.update(frames, timestamps=None)    # list of S PoseResult
        trk.reset(stream=None); trk.tracks(stream); trk.last_frame_kind

    `estimator`: a TopDownPoseEstimator (its `flip_test`, `use_graph`, thresholds and capacity apply unchanged).  `slots`: tracks kept
    at most PER STREAM (capacity .. 256; default: the estimator's capacity, so that every person of a frame finds a slot: one image may take
    every slot of the capacity).  The estimator's `capacity` itself is SHARED by the S images of a call (size it as S x the persons expected
    per image; detections beyond it are dropped from the end of the (image, detection) order and counted in `PoseResult.dropped`), so an
    estimator with a capacity above 256 is refused.  `match_thre`: the least OKS at which a pose continues a track.  `max_age`: calls a
    track survives without being seen.  `detect_every`: a detector frame every that many calls (1: every call).  `box_expand`: the factor a
    propagated box grows about its centre, on top of the key points' extent.  `sigmas`: per-joint OKS sigmas (default COCO's 17; required
    for any other joint count).  `smooth`: a `OneEuro`, or None (the default: no filter, no extra launch, buffer or byte copied).
    ONE frame kind per call, chosen on the host from counters and the previous results only.  A call is a detector frame when it is the
    first call, or the first after reset() of all streams or of any one stream; when `detect_every` calls have passed, counted from the last
    detector frame; or when the previous call returned no person in EVERY stream.  Every other call is propagated: on it a stream without
    live tracks (an empty scene at the last detector frame, say) returns no persons until the next detector frame.  Streams of different
    sizes, streams that skip a call and a `detect_every` per stream are not supported."""

    MAX_GRAPHS = 8

    def __init__(self, estimator, streams: int, slots=None, match_thre: float = 0.5, max_age: int = 30, detect_every: int = 1,
                 box_expand: float = 1.25, sigmas=None, smooth=None):
        if streams != 1 and isinstance(estimator, TopDownPoseEstimator) and estimator.capacity > MAX_SLOTS:
            raise ValueError(f"estimator: capacity {estimator.capacity} exceeds the tracker's limit of {MAX_SLOTS} tracks per stream (one image "
                             f"may take every slot of the capacity, which the streams of a call share); use an estimator with capacity <= {MAX_SLOTS}")
        slots, sigmas = _tracker_args(estimator, slots, match_thre, max_age, detect_every, box_expand, sigmas, smooth)
        if not isinstance(streams, int) or isinstance(streams, bool) or not (1 <= streams <= MAX_STREAMS):
            raise ValueError(f"streams: expected an int in 1..{MAX_STREAMS}, got {streams!r}")
        self.estimator, self.streams, self.slots = estimator, streams, slots
        self.match_thre, self.max_age, self.detect_every, self.box_expand = float(match_thre), max_age, detect_every, float(box_expand)
        self.sigmas, self.smooth = sigmas, smooth
        self._state: Dict[str, torch.Tensor] = {}      # device tensors [streams, ...]: id, age, miss, kps, area, conf, next_id
        self._smooth_state: Dict[str, torch.Tensor] = {}  # device tensors [streams, ...]: id, x, dx, t, n, now
        self._sim = None
        self._now_host = None                          # pinned: the S times on their way to smooth_state["now"]
        self._frame_index = [0] * streams              # per stream, calls since construction or its reset(): the clock without timestamps
        self._graphs: Dict[tuple, tuple] = {}
        self._since_detect, self._prev_n, self._fresh = 0, [0] * streams, True
        self.last_frame_kind = None                    # "detector" / "propagated": what the last update ran

    # -- state --------------------------------------------------------------------------------------------------------------------------
    @property
    def state(self) -> Dict[str, torch.Tensor]:
        """The tracks, in device memory (allocated with the first frame; empty before it)."""
        return self._state

    @property
    def smooth_state(self) -> Dict[str, torch.Tensor]:
        """The smoother's state, in device memory (allocated with the first smoothed frame; empty before it)."""
        return self._smooth_state

    def _ensure_state(self, J: int) -> None:
        if self.sigmas is None and J != 17:
            raise ValueError(f"sigmas: the default OKS sigmas are COCO's 17; the pose model has {J} joints, pass `sigmas`")
        if self.sigmas is not None and self.sigmas.size != J:
            raise ValueError(f"sigmas: {self.sigmas.size} values for a pose model with {J} joints")
        dev, S, n = self.estimator.device, self.streams, self.slots
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        if self.smooth is not None and not (self._smooth_state and self._smooth_state["n"].shape[2] == J):
            self._smooth_state = {"id": z((S, n), torch.int32), "x": z((S, n, J, 2), torch.float64), "dx": z((S, n, J, 2), torch.float64),
                                  "t": z((S, n, J), torch.float64), "n": z((S, n, J), torch.int32), "now": z((S,), torch.float64)}
            self._now_host = torch.zeros((S,), dtype=torch.float64).pin_memory()
            self._graphs.clear()
        if self._state and self._state["kps"].shape[2] == J:
            return
        self._state = {"id": z((S, n), torch.int32), "age": z((S, n), torch.int32), "miss": z((S, n), torch.int32),
                       "kps": z((S, n, J, 3), torch.float64), "area": z((S, n), torch.float64), "conf": z((S, n), torch.float32),
                       "next_id": z((S,), torch.int32)}
        self._sim = z((S, n, n), torch.float64)
        self._sig = None if self.sigmas is None else (ctypes.c_double * J)(*self.sigmas.tolist())
        self._graphs.clear()
        self.reset()

    def _check_stream(self, stream) -> int:
        if not isinstance(stream, int) or isinstance(stream, bool) or not (0 <= stream < self.streams):
            raise ValueError(f"stream: expected an int in 0..{self.streams - 1}, got {stream!r}")
        return stream

    def reset(self, stream=None) -> None:
        """Forget every track of every stream (`stream=None`) or of one stream: its ids restart at 1, its smoother and its clock of
        updates without timestamps start again, and the next call is a detector frame for all streams (the other streams keep their
        tracks through it)."""
        which = range(self.streams) if stream is None else (self._check_stream(stream),)
        for s in which:
            for k, t in self._state.items():
                t[s].fill_(1) if k == "next_id" else t[s].zero_()
            for t in self._smooth_state.values():
                t[s].zero_()
            self._frame_index[s], self._prev_n[s] = 0, 0
        self._fresh = True

    def tracks(self, stream) -> Dict[str, np.ndarray]:
        """A host copy of one stream's live tracks (id, age, miss, keypoints, area, conf), in slot order.  For inspection: it synchronises."""
        s = self._check_stream(stream)
        if not self._state:
            return {k: np.zeros(0) for k in ("id", "age", "miss", "keypoints", "area", "conf")}
        h = {k: v[s].cpu().numpy() for k, v in self._state.items() if k != "next_id"}
        live = h["id"] != 0
        return {"id": h["id"][live], "age": h["age"][live], "miss": h["miss"][live], "keypoints": h["kps"][live], "area": h["area"][live],
                "conf": h["conf"][live]}

    # -- the frame kind: host counters only, no device call ---------------------------------------------------------------------------------
    def _next_is_detector(self) -> bool:
        """The kind of the coming call (see the class docstring)."""
        return self._fresh or self._since_detect >= self.detect_every or not any(self._prev_n)

    def _ran(self, detect: bool, counts) -> None:
        """The call ran as `detect` says and returned counts[s] persons in stream s."""
        self._since_detect = 1 if detect else self._since_detect + 1
        self._prev_n, self._fresh = list(counts), False
        self.last_frame_kind = "detector" if detect else "propagated"

    # -- the two frames -----------------------------------------------------------------------------------------------------------------
    def _boxes(self, fr: _Frame, J: int) -> None:
        est, st = self.estimator, self._state
        _lib.check(_lib.lib().sp_track_boxes_images(P(st["id"]), P(st["miss"]), P(st["kps"]), P(st["conf"]), self.streams, self.slots, J,
                                                    est.in_vis_thre, self.box_expand, float(max(est.person_cls, 0)), fr.W, fr.H, fr.max_det,
                                                    P(fr.det), P(fr.counts), _lib.current_stream(est.device)), "sp_track_boxes_images")

    def _associate(self, fr: _Frame, J: int) -> None:
        est, st = self.estimator, self._state
        _lib.check(_lib.lib().sp_track_associate_images(P(fr.kps64), P(fr.area), P(fr.box), P(fr.keep), P(fr.keep_count), P(fr.seg), self.streams,
                                                        est.capacity, J, self._sig, self.match_thre, self.max_age, self.slots, P(st["id"]),
                                                        P(st["age"]), P(st["miss"]), P(st["kps"]), P(st["area"]), P(st["conf"]), P(st["next_id"]),
                                                        P(self._sim), P(fr.track_id), _lib.current_stream(est.device)),
                   "sp_track_associate_images")

    def _smooth(self, fr: _Frame, J: int) -> None:
        """sp_track_smooth_images on what the association just left in the frame; the kernel reads the S times from smooth_state["now"]."""
        est, sm, ss = self.estimator, self.smooth, self._smooth_state
        _lib.check(_lib.lib().sp_track_smooth_images(P(fr.kps64), P(fr.box), P(fr.track_id), P(fr.keep), P(fr.keep_count), P(fr.seg), self.streams,
                                                     est.capacity, J, P(self._state["id"]), self.slots, P(ss["now"]), sm.min_cutoff, sm.beta,
                                                     sm.d_cutoff, sm.max_gap, est.in_vis_thre, P(ss["id"]), P(ss["x"]), P(ss["dx"]), P(ss["t"]),
                                                     P(ss["n"]), P(fr.kps_smooth), _lib.current_stream(est.device)), "sp_track_smooth_images")

    def _launch(self, fr: _Frame, detect: bool, det_prog, pose_prog, single_stream: bool, warm_up: bool = False) -> None:
        """The call's launches.  `warm_up`: the run ahead of a capture, which is there for what allocates (the programs' pools, the
        workspaces).  It leaves out the tracker's own kernels: they allocate nothing, and the association and the smoother must advance
        the tracks once per call; the overlay changes no state, whatever ids and smoothed poses the frame holds."""
        est, J = self.estimator, pose_prog.out_shape[0]
        if detect:
            est._detect(fr, det_prog, single_stream)
        elif not warm_up:
            self._boxes(fr, J)
        est._poses(fr, pose_prog, single_stream)
        if not warm_up:
            self._associate(fr, J)
            if self.smooth is not None:
                self._smooth(fr, J)
        # (nothing without estimator.renderer / .redactor) the frame's ids colour the persons; a smoothing tracker draws the smoothed
        # poses, while a redactor always hides what this frame's raw key points say
        est._render(fr, J, tracked=True, kps=None if self.smooth is None else fr.kps_smooth)

    def _params(self, det_prog, pose_prog) -> tuple:
        return (self.estimator._params(det_prog, pose_prog), self.match_thre, self.max_age, self.box_expand, self.slots, id(self._sim),
                None if self.smooth is None else self.smooth.key() + (id(self._smooth_state["n"]),))

    def _graph(self, fr: _Frame, detect: bool, det_prog, pose_prog):
        key = (fr.B, fr.H, fr.W, detect, None if self.smooth is None else self.smooth.key())
        entry = self._graphs.get(key)
        params = self._params(det_prog, pose_prog)
        if entry is not None and entry[0] is fr and entry[2] == params:
            self._graphs[key] = self._graphs.pop(key)  # most recently used last
            fr.hm = entry[3][5]                      # the heat maps THIS graph writes (the frame's other graph, or an eager run, left its own)
            return entry[1]
        est = self.estimator
        graph = capture_graph(est.device, lambda: self._launch(fr, detect, det_prog, pose_prog, True, warm_up=True),
                              lambda: self._launch(fr, detect, det_prog, pose_prog, True))
        # the nodes hold raw pointers into both programs' activation pools for the batch sizes used: keep them alive
        # (and, with a heat overlay on the estimator, the heat maps of the captured run: fr.hm, None without one)
        keepalive = (pose_prog, pose_prog.pool_for(est._pose_batch(), est.device), self._state, self._sim, self._smooth_state, fr.hm) + \
            est._det_keepalive(fr, det_prog)
        self._graphs.pop(key, None)
        if len(self._graphs) >= self.MAX_GRAPHS:
            self._graphs.pop(next(iter(self._graphs)))
        self._graphs[key] = (fr, graph, params, keepalive)
        return graph

    @torch.no_grad()
    def update(self, frames, timestamps=None):
        """The next frame of every stream: uint8 BGR [S, H, W, 3] (numpy or CUDA) or a list of S images (or S video.YuvFrames) of one size -> a list of S
        PoseResult with `track_id` (and `keypoints_smooth`, `image`, `jpeg` as the estimator's options add them), stream s's in place s.
        `timestamps`: S finite times in seconds, one per stream, for a tracker that smooths (default: each stream's frame index /
        `smooth.fps`, the index counted from the stream's first frame after construction or reset()).  A time that does not advance is not
        an error: the filter starts again.  A propagated call does not run the detector (see the class docstring)."""
        est, S = self.estimator, self.streams
        times = None
        if timestamps is not None:
            if self.smooth is None:
                raise ValueError("timestamps: this tracker does not smooth (MultiStreamTracker(..., smooth=OneEuro(...))); nothing would read them")
            times = list(timestamps) if isinstance(timestamps, (list, tuple, np.ndarray)) else None
            if times is None or len(times) != S:
                raise ValueError(f"timestamps: expected {S} times in seconds, one per stream, got {timestamps!r}")
            for t in times:
                if not isinstance(t, (int, float, np.integer, np.floating)) or isinstance(t, bool) or not (abs(float(t)) < float("inf")):
                    raise ValueError(f"timestamps: finite times in seconds, got {t!r}")
        if isinstance(frames, (list, tuple)) and len(frames) != S:
            raise ValueError(f"frames: this tracker follows {S} streams, got {len(frames)} images")
        imgs = est._shape_of(frames, batched=True)   # (a list of differently sized images: ValueError; a CPU tensor: HipLibraryError)
        if imgs.shape[0] != S:
            raise ValueError(f"frames: this tracker follows {S} streams, got {imgs.shape[0]} images")
        return self._update(imgs, times)

    def _update(self, imgs, times):
        """update() on checked arguments: the S frames as the estimator's frame takes them, and their times or None."""
        est, S = self.estimator, self.streams
        H, W = imgs.shape[1], imgs.shape[2]
        detect = self._next_is_detector()
        det_prog = None
        if detect:
            det_prog = est._det_program(S, H, W)
        pose_prog = est._pose_program()
        J = pose_prog.out_shape[0]
        self._ensure_state(J)
        fr = est._frame(S, H, W, est.MAX_DET, J, smooth=self.smooth is not None)
        est._stage_caption(fr)                       # (nothing without a caption) ahead of the launch or replay that reads it, as the times below
        est._load(fr, imgs)
        if self.smooth is not None:                  # the S times, on the frame's stream ahead of the launch or replay that reads them
            for s in range(S):
                self._now_host[s] = self._frame_index[s] / self.smooth.fps if times is None else float(times[s])
            self._smooth_state["now"].copy_(self._now_host, non_blocking=True)
        self._frame_index = [i + 1 for i in self._frame_index]
        self._prev_n = [0] * S                       # (a call that raises below is followed by a detector frame)
        if est.use_graph:
            self._graph(fr, detect, det_prog, pose_prog).replay()
        else:
            self._launch(fr, detect, det_prog, pose_prog, False)
        res = est._results(fr, tracked=True, detected=detect)      # (the fetch also ends the copy out of _now_host)
        self._ran(detect, [len(r) for r in res])
        return res


def _stream0(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A one-stream tracker's [1, ...] tensors without the stream axis: views of the same memory (`next_id` and `now` are [1] either way)."""
    return {k: v[0] if v.dim() > 1 else v for k, v in state.items()}


class PoseTracker(MultiStreamTracker):
    """One video stream: MultiStreamTracker with streams=1 - its arguments, its kernels, its frame-kind rule (the first frame, the first
    after reset(), every `detect_every`-th frame counted from the last detector frame, and whenever the previous frame returned no
    person) - taking one image and returning one PoseResult.  `state` and `smooth_state` are the tracker's device memory without the
    stream axis (id [slots], kps [slots, J, 3], next_id [1], x [slots, J, 2], now [1], ...)."""

    def __init__(self, estimator, slots=None, match_thre: float = 0.5, max_age: int = 30, detect_every: int = 1, box_expand: float = 1.25,
                 sigmas=None, smooth=None):
        super().__init__(estimator, 1, slots, match_thre, max_age, detect_every, box_expand, sigmas, smooth)

    state = property(lambda self: _stream0(self._state))
    smooth_state = property(lambda self: _stream0(self._smooth_state))

    def reset(self) -> None:
        """Forget every track: the next frame is a detector frame and ids restart at 1; the smoother starts again, and so does the clock
        of updates without a timestamp."""
        super().reset()

    def tracks(self) -> Dict[str, np.ndarray]:
        """A host copy of the live tracks (id, age, miss, keypoints, area, conf), in slot order.  For inspection: it synchronises."""
        return super().tracks(0)

    @torch.no_grad()
    def update(self, img, timestamp=None) -> PoseResult:
        """One uint8 BGR image [H, W, 3] (numpy or CUDA) or one video.YuvFrame, the next frame of the stream -> the persons in it with
        their `track_id`s.
        A propagated frame (see the module docstring) does not run the detector: new persons appear at the next detector frame.
        `timestamp`: the frame's time in seconds, for a tracker that smooths (default: frame index / `smooth.fps`, the index counted from
        the first frame after construction or reset()).  A time that does not advance is not an error: the filter starts again."""
        if timestamp is not None:
            if self.smooth is None:
                raise ValueError("timestamp: this tracker does not smooth (PoseTracker(..., smooth=OneEuro(...))); nothing would read it")
            if not isinstance(timestamp, (int, float)) or isinstance(timestamp, bool) or not (abs(float(timestamp)) < float("inf")):
                raise ValueError(f"timestamp: a finite time in seconds, got {timestamp!r}")
        img = self.estimator._shape_of(img, batched=False)
        return self._update(img[None], None if timestamp is None else [timestamp])[0]
