"""What the bench tools of the input stores and of the validation pass share (bench_tie_store, bench_report_store,
bench_token_embed, bench_cxr_store, bench_hourly, val_bench): the median, the two ways a time is taken, and the lines a tool prints
and writes to ``--out``.  ONE unit: every timer returns milliseconds; a caller that prints microseconds multiplies where it
formats."""
import os
import time

import torch


def median(xs):
    return sorted(xs)[len(xs) // 2]


def device_ms(fn, n: int) -> float:
    """ms per call by device events around ``n`` calls back to back (an upper bound on a kernel: the window holds the host's
    enqueue of every launch)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def wall_ms(fn, sync: bool = True) -> float:
    """ms of one call by the host clock; ``sync``: the device is idle when the clock starts, and the call ends in a synchronise
    (False: host work alone, or a call that synchronises by itself)"""
    if sync:
        torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    if sync:
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


class Lines:
    """``say = Lines()``: ``say(s)`` prints a line at once and keeps it; ``say.write(path)`` is the tool's ``--out``"""

    def __init__(self):
        self.lines = []

    def __call__(self, s: str):
        print(s, flush=True)
        self.lines.append(s)

    def write(self, path):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(self.lines) + "\n")
