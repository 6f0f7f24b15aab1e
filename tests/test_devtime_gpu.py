"""fasterseg_amd/devtime.py by counting launches, not by comparing times: `issue` increments a 1-element int64 device counter, so the
counter after a call is the number of launches the call put on the device - warm launches, captured copies x replays and bracketed
calls.  (copies, rounds) = (20, 3) is the census and profile() (and what the engine's tuner does in its own copies), (10, 1) the HEFT
profile, (40, 5) / (30, 5) the engine's frame brackets.  Every counter is read on the stream that was current before the call, without a synchronise: the value is final only if the
side stream was joined back into it.  The times are finite and positive; no bound is put on them."""
import math

import pytest
import torch

from fasterseg_amd import devtime

pytestmark = pytest.mark.gpu


def _counter():
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return counter, (lambda st: counter.add_(1)), torch.cuda.current_stream()


def _ok(ms):
    return isinstance(ms, float) and math.isfinite(ms) and ms > 0


@pytest.mark.parametrize("copies,rounds", [(1, 1), (20, 3), (10, 1)])
def test_captured_ms_launch_count(copies, rounds):
    counter, issue, stream = _counter()
    seen = []

    def pick(times):
        seen.append(list(times))
        return min(times)
    ms = devtime.captured_ms(issue, copies=copies, rounds=rounds, pick=pick)
    assert torch.cuda.current_stream() == stream
    assert int(counter.item()) == 1 + copies * (1 + rounds)
    assert _ok(ms)
    assert len(seen) == 1 and len(seen[0]) == rounds and all(_ok(t) for t in seen[0])
    assert ms == min(seen[0]) / copies


def test_captured_ms_defaults_and_median_pick():
    counter, issue, stream = _counter()
    assert _ok(devtime.captured_ms(issue))
    assert int(counter.item()) == 1 + 20 * (1 + 3)
    seen = []

    def median(times):
        seen.append(list(times))
        return sorted(times)[len(times) // 2]
    ms = devtime.captured_ms(issue, copies=4, rounds=5, pick=median)
    assert torch.cuda.current_stream() == stream
    assert int(counter.item()) == 81 + 1 + 4 * (1 + 5)
    assert len(seen[0]) == 5 and ms == sorted(seen[0])[2] / 4


def test_captured_ms_on_a_given_stream_without_warm_launch():
    """profile()'s form: the caller owns the side stream, has warmed already, and joins it when it is done with it"""
    counter, issue, stream = _counter()
    side = torch.cuda.Stream()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        issue(None)
        side.synchronize()
    for n in (1, 2):
        assert _ok(devtime.captured_ms(issue, copies=3, rounds=2, stream=side, warm=False))
        assert torch.cuda.current_stream() == stream
        stream.wait_stream(side)
        assert int(counter.item()) == 1 + n * 3 * (1 + 2)


@pytest.mark.parametrize("copies", [1, 20])
def test_capture_launch_count(copies):
    counter, issue, stream = _counter()
    handles = []
    g = devtime.capture(lambda st: (handles.append(st.value), issue(st)), copies)
    assert torch.cuda.current_stream() == stream
    assert int(counter.item()) == 1
    g.replay()
    assert int(counter.item()) == 1 + copies
    g.replay()
    assert int(counter.item()) == 1 + 2 * copies
    # one warm call and `copies` captured ones, each handed the side stream's handle: not the caller's stream
    assert len(handles) == 1 + copies and len(set(handles)) == 1 and handles[0] != stream.cuda_stream


@pytest.mark.parametrize("n,warm", [(40, 5), (1, 0), (30, 5)])
@pytest.mark.parametrize("sync", [True, False])
def test_block_ms_launch_count(n, warm, sync):
    counter, issue, stream = _counter()
    ms = devtime.block_ms(lambda: issue(None), n, warm=warm, sync=sync)
    assert torch.cuda.current_stream() == stream
    assert int(counter.item()) == warm + n
    assert _ok(ms)


def test_block_ms_replays_a_captured_graph():
    """the engine's frame bracket (`_time_graph`): 5 warm replays, no synchronise, one bracket round `reps` replays"""
    counter, issue, _ = _counter()
    g = devtime.capture(issue, 3)
    assert _ok(devtime.block_ms(g.replay, 4, warm=5, sync=False))
    assert int(counter.item()) == 1 + 3 * (5 + 4)
