"""Making stream ordering visible (tests/test_gpu_streams.py).

On the null stream every launch of the library is serialised behind the one before, so a launch that the library puts on the
wrong stream, or in front of the wait it needs, computes the right numbers anyway.  Here the caller's streams are
torch.cuda.Stream() objects - created non-blocking, nothing orders them against the null stream or one another - and a pure
delay (`busy`) is queued in front of the work under test: a misplaced launch then runs early by tens of milliseconds, not by
nanoseconds, and reads memory that has not been written yet.

A test that uses a delay states what the delay has to achieve, and fails (never skips) when it did not:
  * `assert_busy(stream)`: after the calls under test have returned the delayed stream is still busy - otherwise the calls
    were ordered by the host's pace alone and the test proved nothing;
  * `Marker`: a one-element fill_ plus an event on the second stream completes while the first stream is still delayed -
    otherwise the two streams share a hardware queue and are not concurrent (`concurrent_pair` draws pairs until one is).

torch is imported when this module is (at collection, before any test loads the HIP library), so that the process holds one
HIP runtime - torch's - and a torch stream handle means the same thing to the library; `one_hip_runtime` checks it."""
import torch

DELAY_MS = 50.              # what a test starts from (and, as measured, what is enough: DESIGN.md)
MAX_DELAY_MS_PER_TEST = 500.
MAX_STREAMS = 6             # caller streams alive at once

_cycles_per_ms = None
_live_streams = 0


def one_hip_runtime():
    """the HIP runtime libraries mapped into this process (there must be one: a stream of one runtime is a wild pointer to
    another)"""
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                paths.add(line.split()[-1])
    assert len(paths) == 1, "more than one HIP runtime is loaded (%s): torch must be imported before the library" % sorted(paths)


def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond, measured once per session with two events"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        assert hasattr(torch.cuda, "_sleep"), "this torch has no torch.cuda._sleep"
        one_hip_runtime()
        st = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 4000000
        with torch.cuda.stream(st):
            torch.cuda._sleep(probe)                # (the first launch loads the kernel)
            for _ in range(2):                      # the second measurement is the one kept
                e0.record(st)
                torch.cuda._sleep(probe)
                e1.record(st)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
        assert ms > 0
        _cycles_per_ms = probe / ms
        print("stream_helpers: torch.cuda._sleep runs %.0f cycles per ms (%d cycles took %.3f ms)" % (_cycles_per_ms, probe, ms))
        with torch.cuda.stream(st):                 # ... and a whole delay, once, to see that the scale holds that far
            e0.record(st)
            torch.cuda._sleep(int(_cycles_per_ms * DELAY_MS))
            e1.record(st)
            e1.synchronize()
        print("stream_helpers: a delay of %.0f ms took %.2f ms" % (DELAY_MS, e0.elapsed_time(e1)))
    return _cycles_per_ms


class Streams:
    """The caller streams of one test and its budget of delays."""

    def __init__(self):
        self.delayed_ms = 0.
        self.mine = []

    def new(self):
        global _live_streams
        assert _live_streams < MAX_STREAMS, "more than %d caller streams alive" % MAX_STREAMS
        _live_streams += 1
        st = torch.cuda.Stream()
        self.mine.append(st)
        return st

    def busy(self, stream, ms=DELAY_MS):
        """queue a pure delay of `ms` milliseconds on `stream`"""
        self.delayed_ms += ms
        assert self.delayed_ms <= MAX_DELAY_MS_PER_TEST, "the delays of one test exceed %.0f ms" % MAX_DELAY_MS_PER_TEST
        cycles = int(cycles_per_ms() * ms)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
        print("stream_helpers: delay of %.0f ms (%d cycles) queued" % (ms, cycles))

    def release(self):
        global _live_streams
        for st in self.mine:
            st.synchronize()
        _live_streams -= len(self.mine)
        self.mine = []


def handle(stream):
    """what capi.*(stream=...) takes"""
    return stream.cuda_stream


def assert_busy(stream, what):
    assert stream.query() is False, "%s: the delayed stream had already drained - the delay ordered nothing" % what


class Marker:
    """a one-element fill_ and an event on `stream`, queued now"""

    def __init__(self, stream):
        self.event = torch.cuda.Event()
        with torch.cuda.stream(stream):
            self.cell = torch.zeros(1, device="cuda")
            self.cell.fill_(1.)
            self.event.record(stream)

    def done_while_busy(self, delayed):
        """waits for the marker (at most as long as the other stream's delay, when the two share a hardware queue), then says
        whether `delayed` was still busy"""
        self.event.synchronize()
        return delayed.query() is False


def concurrent_pair(streams, draws=8, ms=20.):
    """Two streams of which the second runs while the first is delayed: the first of up to `draws` pairs that shows it (a
    process has few hardware queues, so two streams may share one).  Costs `ms` of delay per pair drawn."""
    global _live_streams
    for n in range(draws):
        a, b = streams.new(), streams.new()
        streams.busy(a, ms)
        ok = Marker(b).done_while_busy(a)
        a.synchronize()
        if ok:
            print("stream_helpers: stream pair %d of at most %d runs side by side" % (n + 1, draws))
            return a, b
        streams.mine.remove(a)
        streams.mine.remove(b)
        _live_streams -= 2
        del a, b
    raise AssertionError("none of %d stream pairs ran concurrently: every second stream waited for the first one's delay" % draws)
