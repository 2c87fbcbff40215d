"""Stream capture into a hipGraph, and the way out of a capture that failed: the one place of the package that captures.
Its users are the pre-training step (train.PretrainTrainer), the inference navigation steps (nav_static.NavGraphRunner)
and the segments of a training rollout (nav_static.NavTrainRunner); they decide when to capture and replay what they get."""
import torch

from . import lib
from .ops_core import ATTN_BITS, Branches
from .ops_reduce import ReduceQueue, WgradStream


class CaptureFailed(RuntimeError):
    """``capture`` could not record its body; ``__cause__`` is the first exception, ``message`` its short form."""

    def __init__(self, cause):
        self.message, self.__cause__ = f"{type(cause).__name__}: {cause}"[:400], cause
        super().__init__(self.message)


def join_captured_side_streams(extra=()):
    """Recovery step of a FAILED stream capture: make the capturing (current) stream wait for every side stream that was
    forked into the capture (keep-bit stream, model-branch stream, weight-gradient streams, the reducer's stream).
    hipStreamEndCapture refuses to end a capture with unjoined forks (hipErrorStreamCaptureUnjoined) and -- on ROCm 7.2 --
    then leaves the origin stream IN capture mode, so that every later launch of the process fails; with the forks
    joined the capture ends normally and its graph is simply dropped."""
    if not torch.cuda.is_available() or not torch.cuda.is_current_stream_capturing():
        return 0
    cur = torch.cuda.current_stream()
    seen, n = {cur.cuda_stream}, 0
    cands = [ATTN_BITS.stream] + list(Branches._streams.values()) + list(WgradStream.streams) + list(extra)
    for st in cands:
        if st is None or st.cuda_stream in seen:
            continue
        seen.add(st.cuda_stream)
        with torch.cuda.stream(st):
            capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            cur.wait_stream(st)
            n += 1
    return n


def abandon(why=""):
    """After a capture that failed and was ended: leave nothing of it behind.  ``why`` goes into the error message."""
    lib.load().bevbert_hip_error_reset()         # the capture's error code must not surface in the next launch check
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the failed hipGraph capture could not be ended: the stream is still capturing and the "
                           f"process cannot issue work any more ({why})")
    torch.cuda.synchronize()
    # host state the aborted capture left behind points into its dead memory pool: deferred weight-gradient closures and
    # queued reduction records -- forget them (what else the caller queued -- collective work handles -- is the caller's)
    WgradStream.drop_pending()
    ReduceQueue.drop_pending()


def capture(body, pool=None, extra_streams=()):
    """Record ``body()`` into a hipGraph of the memory pool ``pool`` (None: a new one; ``graph.pool()`` names it for the
    captures that are to share it) and return ``(graph, what body returned)``; nothing has executed, the caller replays.
    ``extra_streams``: side streams the body may fork beyond those ``join_captured_side_streams`` knows.

    A body that raises does so INSIDE the capture: its forks are joined there so that the capture can end (see
    ``join_captured_side_streams``), then ``abandon`` clears up and ``CaptureFailed`` is raised; the caller goes on eagerly.

    Thread-local capture mode: other threads of the process keep making HIP calls while this one captures -- the loader's
    producer thread allocates pinned staging buffers and device buffer sets (loader.BucketManager), and
    ProcessGroupNCCL's watchdog polls the completion events of earlier eager collectives; in "global" mode any such call
    invalidates the capture (hipErrorStreamCaptureInvalidated; seen in round 4 with the first pin_memory() of a buffer
    set).  Calls made by THIS thread and by autograd's backward thread on its behalf are still checked."""
    torch.cuda.synchronize()
    if pool is None:
        pool = torch.cuda.graph_pool_handle()
    graph = torch.cuda.CUDAGraph()
    err = result = None
    try:
        with torch.cuda.graph(graph, pool=pool, capture_error_mode="thread_local"):
            try:
                result = body()
            except Exception as e:      # noqa: BLE001 -- still inside the capture
                err = e
                join_captured_side_streams(extra_streams)
    except Exception as e:      # noqa: BLE001 -- ending the capture failed as well
        err = err or e
    if err is None:
        return graph, result
    failed = CaptureFailed(err)
    abandon(failed.message)
    raise failed


class StaticInputs:
    """The static input buffers of a captured step: ``bufs`` holds one per tensor of ``feeds``, of the shape ``shapes``
    names for it (default: the tensor's own).  A smaller tensor fills the leading corner; the padding stays zero."""

    def __init__(self, feeds, shapes):
        self.bufs = {k: torch.zeros(shapes.get(k, v.shape), dtype=v.dtype, device=v.device) for k, v in feeds.items()}
        self.filled = {}          # name -> shape of the last tensor written into the buffer

    def fill(self, name, v):
        buf = self.bufs[name]
        if v.shape != buf.shape:
            last = self.filled.get(name)
            if last is not None and any(l > n for l, n in zip(last, v.shape)):
                buf.zero_()       # the tensor shrank (a new episode's map): clear what the last, wider fill left behind
            buf = buf[tuple(slice(0, n) for n in v.shape)]
        buf.copy_(v, non_blocking=True)
        self.filled[name] = tuple(v.shape)
