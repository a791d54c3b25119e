"""Detector for work that lands on the wrong stream (used by tests/test_streams_gpu.py over tests/stream_cases.py).

On torch's default (legacy null) stream every launch is ordered after every other, whatever stream argument it was given, so
a launch that forgot its stream, a null-stream memset, a missing event join or a buffer recycled under a running kernel cannot
be seen there.  Here the call under test runs on a non-blocking side stream BEHIND a delay kernel and behind the copies that
bring its real inputs (A) into buffers that so far hold valid decoy inputs (B):

    expected = op(A) on the default stream                         (step 1)
    prime    = op(inp = B) on the side stream, synchronised        (step 2: every cached scratch now holds B's intermediates)
    on the side stream: delay; gate = event; inp.copy_(A); r = op(inp); clone the leaves; synchronise   (step 3)

Anything that runs ahead of the side stream reads B (or B's intermediates) and the result differs from ``expected`` in at
least one bit.  ``syncs=False`` cases also assert that the gate has not fired when ``op`` returns: the call did not block
the host (step 4), and the delay was long enough to prove it.  The control (step 5) issues ``op`` under the DEFAULT stream
while the delay and the copies stay on the side stream: it must finish before A arrives and must differ from ``expected``,
which shows that the detector can fail for this case's data.

The leaf walker and the bit comparison work on CPU tensors and are unit-tested without a GPU (tests/test_stream_cases_args.py).
"""
from __future__ import annotations

import time
from typing import Callable, NamedTuple

import torch

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Case(NamedTuple):
    """One row of the table.  ``make(device)`` builds the stateful objects and returns ``(op, A, B)``: ``op(inputs) -> result``
    and two dicts of device tensors with the same keys, shapes and dtypes, both valid inputs.  ``covers``: the public entries
    the case runs.  ``syncs``: whether the call reads something back to the host.  ``control=False`` only for cases without
    a device input."""
    name: str
    covers: tuple
    make: Callable
    syncs: bool
    control: bool = True


# ---------------------------------------------------------------------------------------------- leaves and comparison
class Flat(dict):
    """A result already flattened to {leaf path: leaf} (``clone_leaves``); ``leaves`` returns its items as they are."""


def leaves(obj, path: str = "r"):
    """[(path, leaf)] of a result: tensors and Python scalars (None, bool, int, float, str) are leaves; tuples, lists,
    NamedTuples, dicts and plain result objects (their public attributes) are walked in a fixed order."""
    if isinstance(obj, Flat):
        return list(obj.items())
    if torch.is_tensor(obj) or obj is None or isinstance(obj, (bool, int, float, str)):
        return [(path, obj)]
    if isinstance(obj, tuple) and hasattr(obj, "_fields"):
        return [x for f in obj._fields for x in leaves(getattr(obj, f), f"{path}.{f}")]
    if isinstance(obj, (tuple, list)):
        return [x for i, v in enumerate(obj) for x in leaves(v, f"{path}[{i}]")]
    if isinstance(obj, dict):
        return [x for k in sorted(obj, key=repr) for x in leaves(obj[k], f"{path}[{k!r}]")]
    if hasattr(obj, "__dict__"):
        return [x for k in sorted(vars(obj)) if not k.startswith("_") for x in leaves(getattr(obj, k), f"{path}.{k}")]
    raise TypeError(f"{path}: a {type(obj).__name__} is not a result leaf")


def _bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's elements as integers of the same width on the CPU (NaN compares equal to the same NaN)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bool:
        return t.reshape(-1).to(torch.uint8)
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    return t.reshape(-1).view(_INT_VIEW[t.element_size()])


def differences(got, want) -> list:
    """One line per difference between two results, each with its leaf path; empty when they are the same bit for bit."""
    lg, lw = leaves(got), leaves(want)
    if [p for p, _ in lg] != [p for p, _ in lw]:
        return [f"leaf structure differs: {[p for p, _ in lg]} != {[p for p, _ in lw]}"]
    out = []
    for (p, g), (_, w) in zip(lg, lw):
        if torch.is_tensor(g) != torch.is_tensor(w):
            out.append(f"{p}: {type(g).__name__} != {type(w).__name__}")
        elif not torch.is_tensor(g):
            same = type(g) is type(w) and (g == w or (isinstance(g, float) and g != g and w != w))
            if not same:
                out.append(f"{p}: {g!r} != {w!r}")
        elif g.dtype != w.dtype:
            out.append(f"{p}: dtype {g.dtype} != {w.dtype}")
        elif tuple(g.shape) != tuple(w.shape):
            out.append(f"{p}: shape {tuple(g.shape)} != {tuple(w.shape)}")
        else:
            bg, bw = _bits(g), _bits(w)
            bad = torch.nonzero(bg != bw).reshape(-1)
            if bad.numel():
                i = int(bad[0])
                out.append(f"{p}: {bad.numel()} of {bg.numel()} elements differ, first at flat index {i}: "
                           f"bits {int(bg[i]) & ((1 << 8 * bg.element_size()) - 1):#x} != "
                           f"{int(bw[i]) & ((1 << 8 * bw.element_size()) - 1):#x}")
    return out


def assert_same(got, want, what: str = "") -> None:
    diff = differences(got, want)
    assert not diff, f"{what}: " + "; ".join(diff[:6])


def to_host(result):
    """The result with every tensor leaf copied to the CPU: the kept bits."""
    if torch.is_tensor(result):
        return result.detach().cpu().clone()
    if result is None or isinstance(result, (bool, int, float, str)):
        return result
    if isinstance(result, tuple) and hasattr(result, "_fields"):
        return type(result)(*[to_host(v) for v in result])
    if isinstance(result, (tuple, list)):
        return type(result)(to_host(v) for v in result)
    if isinstance(result, dict):
        return type(result)((k, to_host(v)) for k, v in result.items())
    return {k: to_host(v) for k, v in vars(result).items() if not k.startswith("_")}


def clone_leaves(result):
    """Every tensor leaf cloned on the current stream, the structure flattened to {path: leaf}."""
    return Flat((p, v.clone() if torch.is_tensor(v) else v) for p, v in leaves(result))


# ---------------------------------------------------------------------------------------------- the delay
_cycles_per_ms = None
STATS = {"longest_enqueue_ms": 0.0, "longest_delay_ms": 0.0}
_MIN_DELAY_MS, _MAX_DELAY_MS = 20.0, 1000.0


def cycles_per_ms() -> float:
    """``torch.cuda._sleep`` cycles per millisecond, measured once per session with events on the default stream."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        cycles = 1_000_000
        while True:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0 or cycles >= 1 << 40:
                break
            cycles *= 8
        _cycles_per_ms = cycles / ms
        print(f"[streams] torch.cuda._sleep: {_cycles_per_ms:.0f} cycles per ms ({cycles} cycles took {ms:.2f} ms); "
              f"base delay {_MIN_DELAY_MS:.0f} ms")
    return _cycles_per_ms


def delay(ms: float) -> None:
    """A single-wave spin of about ``ms`` on the current stream."""
    torch.cuda._sleep(int(ms * cycles_per_ms()))


def _note(enqueue_ms: float, delay_ms: float) -> None:
    if enqueue_ms > STATS["longest_enqueue_ms"] or delay_ms > STATS["longest_delay_ms"]:
        STATS["longest_enqueue_ms"] = max(STATS["longest_enqueue_ms"], enqueue_ms)
        STATS["longest_delay_ms"] = max(STATS["longest_delay_ms"], delay_ms)
        print(f"[streams] longest host enqueue so far {STATS['longest_enqueue_ms']:.2f} ms, longest delay "
              f"{STATS['longest_delay_ms']:.0f} ms")


_independent = {}


def independent_streams(device, want: int = 3, tries: int = 16) -> list:
    """Side streams on which a spin does NOT hold up the default stream, found once per session.  A process has a few
    hardware queues (four by default) and the runtime spreads its streams over them; a side stream that shares its queue with
    the default stream serialises with it in hardware, whatever the streams' flags say, and a control on such a stream could
    not tell a wrong-stream launch from a right one.  Each candidate is probed: a 5 ms spin and a gate on it, a small fill on
    the default stream, the default stream synchronised - the gate must not have fired."""
    key = str(device)
    if key not in _independent:
        found, probe = [], torch.zeros(64, device=device)
        for _ in range(tries):
            s = torch.cuda.Stream(device)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                delay(5.0)
                gate = torch.cuda.Event()
                gate.record()
            probe.add_(1.0)
            torch.cuda.default_stream(device).synchronize()
            if not gate.query():
                found.append(s)
            s.synchronize()
            if len(found) == want:
                break
        print(f"[streams] {len(found)} side streams found whose queue the default stream does not share")
        _independent[key] = found
    return _independent[key]


_LENGTHEN = ("the gate fired before the call under test had returned: lengthen the delay (stream_harness._MIN_DELAY_MS / "
             "_MAX_DELAY_MS) - the run proves nothing as it is")


class Built:
    """A case made ready: its op, A, B, the decoy-holding input buffers, the expected bits and the delay this case needs
    (at least the base delay, and four times what the primed call took from first enqueue to completion)."""

    def __init__(self, case: Case, device):
        self.case = case
        self.op, self.A, self.B = case.make(device)
        assert set(self.A) == set(self.B), case.name
        for k in self.A:
            a, b = self.A[k], self.B[k]
            assert a.shape == b.shape and a.dtype == b.dtype and a.is_cuda and b.is_cuda, (case.name, k)
        torch.cuda.synchronize()
        self.expected = to_host(clone_leaves(self.op(self.A)))                     # step 1, default stream
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream(device)
        self.inp = {k: v.clone() for k, v in self.B.items()}
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):                                        # step 2: prime with B
            t0 = time.perf_counter()
            self.op(self.inp)
            self.stream.synchronize()
            took = (time.perf_counter() - t0) * 1e3
        self.delay_ms = min(max(_MIN_DELAY_MS, 4.0 * took), _MAX_DELAY_MS)

    def _gate_and_copies(self):
        delay(self.delay_ms)
        gate = torch.cuda.Event()
        gate.record()
        for k, v in self.inp.items():
            v.copy_(self.A[k])
        return gate

    def _reset(self):
        for k, v in self.inp.items():
            v.copy_(self.B[k])
        torch.cuda.synchronize()

    def under_test(self):
        """Step 3 (and 4): the result of ``op`` on the side stream behind the delay and the copies of A."""
        self._reset()
        s = self.stream
        with torch.cuda.stream(s):
            gate = self._gate_and_copies()
            t0 = time.perf_counter()
            r = self.op(self.inp)
            returned_early = not gate.query()
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            kept = clone_leaves(r)
            s.synchronize()
        if not self.case.syncs:
            _note(enqueue_ms, self.delay_ms)
            assert returned_early, (f"{self.case.name}: declared syncs=False, but the gate behind a {self.delay_ms:.0f} ms delay had "
                                    f"fired when the call returned after {enqueue_ms:.2f} ms on the host: either the call blocks "
                                    f"the host (a finding), or " + _LENGTHEN)
        return to_host(kept)

    def control(self):
        """Step 5: ``op`` issued under the default stream, the delay and the copies on a side stream whose hardware queue the
        default stream does not share (``independent_streams``).  The op's own internal streams may still share a queue with
        that side stream and wait behind the spin; then the next candidate stream is taken.  The result counts only from a
        run whose gate had not fired when the default stream was done."""
        candidates = independent_streams(self.stream.device)
        assert candidates, "no side stream was found that runs beside the default stream: the control cannot be made"
        for s in candidates:
            self._reset()
            with torch.cuda.stream(s):
                gate = self._gate_and_copies()
            r = self.op(self.inp)                                                   # default stream: ahead of A
            kept = clone_leaves(r)
            torch.cuda.default_stream(s.device).synchronize()
            early = not gate.query()
            s.synchronize()
            if early:
                return to_host(kept)
        raise AssertionError(f"{self.case.name}: control: " + _LENGTHEN)
