"""Deterministic delay injection for the stream-ordering tests (a test helper, not a conftest).

Every GPU test synchronises before it reads a result, which hides a reader that runs ahead of its writer on another stream.  `delayed()`
makes one side of the step's fork late on purpose: in front of every `harp_*` launch that takes a stream, it enqueues a calibrated busy
wait (`torch.cuda._sleep`) on that launch's stream.  A missing edge between two streams then shows on every run instead of when the
hardware happens to interleave them badly."""
import contextlib
import os
import re

import torch

from harp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET_US = 300.0                                   # well above any single kernel of the step at S = 128, B = 3
_cal = {}


def stream_entry_points():
    """names of the C-ABI functions whose declaration in include/harp_hip.h ends in `hipStream_t stream`"""
    with open(os.path.join(ROOT, "include", "harp_hip.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    names = [n for n, args in re.findall(r"\b(harp_\w+)\s*\(([^;{]*?)\)\s*;", src) if re.search(r"hipStream_t\s+stream$", args.strip())]
    assert len(names) > 50, names                     # (the parser still finds the header's launches)
    return names


def _time_us(fn, reps=5):
    """median wall time of fn() on the current stream, CUDA events"""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[len(ts) // 2]


def _sleep_fn():
    """(n -> enqueue a busy wait of n units on the current stream, what the unit is): torch's clock64 spin kernel, or — where that is
    unusable — a chain of n dependent element-wise kernels on a scratch tensor"""
    try:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        return torch.cuda._sleep, "clock64 cycles"
    except Exception:
        scratch = torch.zeros(1 << 16, device="cuda")

        def chain(n):
            for _ in range(int(n)):
                scratch.mul_(1.0)
        return chain, "element-wise launches"


def calibrate():
    """(sleep function, n, measured µs): n units of the busy wait take about TARGET_US.  How clock64 maps to wall time on the device is
    measured here, not assumed (once per process)."""
    if not _cal:
        sleep, unit = _sleep_fn()
        n1 = 20000 if unit.startswith("clock") else 4
        _time_us(lambda: sleep(n1), 2)                  # (first launch: code-object load)
        t1, t2 = _time_us(lambda: sleep(n1)), _time_us(lambda: sleep(2 * n1))
        per = max(t2 - t1, 1e-3) / n1
        n = max(1, int(round(TARGET_US / per)))
        us = _time_us(lambda: sleep(n))
        print(f"[delay] {n} {unit} -> {us:.0f} us ({per * 1e3:.3f} ns per unit)")
        assert 100.0 <= us <= 2000.0, (n, unit, us)
        _cal.update(sleep=sleep, n=n, us=us, unit=unit)
    return _cal["sleep"], _cal["n"], _cal["us"]


@contextlib.contextmanager
def delayed(eng, where):
    """Inside the context, every stream launch of the C ABI that runs on the step's second (and further) streams — where="side" — or on
    its main stream — where="main" — waits the calibrated delay first.  The main stream is the stream current when `eng.forward_backward`
    was last entered (under capture: torch's capture stream).  "side" makes every side-branch producer late: it catches a main-stream
    reader without a join.  "main" makes the main-stream producers late: it catches a side-stream reader without a wait.  Captured graphs
    do not contain the delays: the engine's graph cache is emptied on entry and on exit."""
    assert where in ("side", "main"), where
    sleep, n, _ = calibrate()
    L = _lib.lib()
    state = {"main": None}
    side = where == "side"

    def wrap(fn):
        def call(*args):
            m = state["main"]
            if m is not None and (torch.cuda.current_stream().cuda_stream != m) == side:
                sleep(n)
            return fn(*args)
        return call

    saved = {name: getattr(L, name) for name in stream_entry_points()}
    fb = eng.forward_backward

    def forward_backward(*args, **kw):
        state["main"] = torch.cuda.current_stream().cuda_stream
        return fb(*args, **kw)

    for name, fn in saved.items():
        setattr(L, name, wrap(fn))
    eng.forward_backward = forward_backward
    eng._graphs = {}
    try:
        yield
    finally:
        del eng.forward_backward                     # (the instance attribute: the class's method shows again)
        for name, fn in saved.items():
            setattr(L, name, fn)
        eng._graphs = {}
