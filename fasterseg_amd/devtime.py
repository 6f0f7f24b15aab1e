"""Device timing with HIP events: the two brackets behind the device times this project prints (census, latency table, the engine's
profile(), tools/*_timing.py).  The engine's tuner still carries its own copies of both.

block_ms     a host loop of calls between two events: whatever the calls enqueue, per call, Python between them included (a whole
             graph replay or a frame per call, where the host keeps ahead of the device).
captured_ms  the launches copied back to back into a throw-away hipGraph whose replay is bracketed: kernel duration plus one
             dependent-launch boundary (~1.5 us) per copy, no Python launch overhead; rocprofv3 --kernel-trace durations of the same
             kernels (profiles/) are the cross-check.
"""
import ctypes

import torch


def block_ms(step, n, warm=0, sync=True):
    """ms per call of `step()` over one event bracket round `n` calls on the current stream, after `warm` unbracketed calls and
    (`sync`) a device synchronise."""
    for _ in range(warm):
        step()
    if sync:
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def capture(issue, copies, stream=None, warm=True):
    """A hipGraph of `copies` back-to-back `issue(st)`, st = the capturing stream's handle (ctypes.c_void_p).  Captured on a fresh
    side stream that waits for the current one and is joined back into it, after one `issue(st)` outside capture (`warm`) that the
    side stream has drained.  A caller that passes `stream` owns the wait and the join."""
    side = stream or torch.cuda.Stream()
    if stream is None:
        side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if warm:
            issue(ctypes.c_void_p(side.cuda_stream))
            side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for _ in range(copies):
                issue(st)
    if stream is None:
        torch.cuda.current_stream().wait_stream(side)
    return g


def captured_ms(issue, copies=20, rounds=3, pick=min, stream=None, warm=True):
    """Device time (ms) of one `issue(st)`: `capture`d `copies` times, replayed once unbracketed, then `rounds` brackets of one
    replay each, all on the side stream; `pick` of the round times (min; a median is `lambda t: sorted(t)[len(t) // 2]`) / copies.
    The graph is dropped on return."""
    side = stream or torch.cuda.Stream()
    if stream is None:
        side.wait_stream(torch.cuda.current_stream())
    g = capture(issue, copies, side, warm)
    with torch.cuda.stream(side):
        g.replay()
        times = [block_ms(g.replay, 1, sync=False) for _ in range(rounds)]
    if stream is None:
        torch.cuda.current_stream().wait_stream(side)
    return pick(times) / copies
