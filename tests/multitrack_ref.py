"""MultiStreamTracker's frame-kind rule on the host, written from its docstring, and PoseTracker's next to it: what the tests of the class
derive the expected kind of every call from.  It imports nothing of the library."""


class FrameKinds:
    """One kind per call for `streams` streams.  A call is a detector frame when it is the first call or the first after a reset (of all
    streams or of one), when `detect_every` calls have passed since the last detector frame, or when the previous call returned no person
    in every stream; every other call is propagated."""

    def __init__(self, streams, detect_every):
        self.streams, self.detect_every = streams, detect_every
        self.since, self.prev, self.fresh = 0, [0] * streams, True

    def reset(self, stream=None):
        for s in (range(self.streams) if stream is None else (stream,)):
            self.prev[s] = 0
        self.fresh = True

    def next(self):
        """-> True when the coming call is a detector frame."""
        return self.fresh or self.since >= self.detect_every or sum(self.prev) == 0

    def done(self, detect, counts):
        """The call ran as `detect` says and returned counts[s] persons in stream s."""
        assert len(counts) == self.streams
        self.since = 1 if detect else self.since + 1
        self.prev, self.fresh = list(counts), False

    @staticmethod
    def name(detect):
        return "detector" if detect else "propagated"


class SingleKinds:
    """PoseTracker's rule: the first frame, the first after reset(), every `detect_every`-th frame counted from the last detector frame,
    and whenever the previous frame returned no person."""

    def __init__(self, detect_every):
        self.detect_every, self.since, self.prev = detect_every, 0, 0

    def reset(self):
        self.since, self.prev = 0, 0

    def next(self):
        return self.prev == 0 or self.since >= self.detect_every

    def done(self, detect, count):
        self.since, self.prev = (1 if detect else self.since + 1), count
