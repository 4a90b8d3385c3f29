"""The stream contract of the C ABI (include/vae_step.h, first paragraph) made testable: a case runs once on the synchronised
default stream and once on a non-default stream that is held up by a chain of matrix products while the host enqueues the
true inputs, the library calls and the read-out behind it.  Before the chain every live buffer holds poison, so work that
is not ordered on the caller's stream (a launch on stream 0, a side stream forked too early or never joined, a copy on the
wrong stream) computes from NaNs or has its result overwritten, and the bits differ from the reference run.

Importing this module touches no GPU; everything that does is inside the functions."""
import gc
import math
import os
import time

import torch

DELAY_MS = 50.0          # the least the chain lasts; over 100 times the 0.23-0.31 ms the one-call step costs the host
MAX_DELAY_MS = 500.0     # no chain is asked to last longer
PYTHON_DELAY_FACTOR = 4  # a case through the Python layer: at least this many times its host time in the reference run
GATE = {"f32": 1e-5, "bf16": 5e-4, "f16": 5e-4}   # relative L2 of the existing parity tests, for outputs two default-stream runs disagree on
POISON_BYTE = 0xA5
RECORD = []              # one dict per case run, in order (written out by the test module when asked to)


class Bufs:
    """The buffers of one run of a case.  live: device inputs and in/out buffers (each with a staging copy of its true value);
    out: pure outputs; inout: the names in `live` whose final contents are compared as well; poison: the valid-but-different
    value an integer input takes (a float input takes NaN)."""

    def __init__(self):
        self.live, self.staging, self.out, self.poison, self.inout, self.keep = {}, {}, {}, {}, [], []
        self.probe = None        # in the delayed run: a function that says whether the stream is still held up
        self.checkpoint = None   # what a case that ends with a read-back by design saw there in front of that read

    def adopt(self, name, tensor, inout=False, poison=None):
        """`tensor` is the live buffer as it stands (a model's flat parameters, ...); its present value is the true one."""
        self.live[name] = tensor
        self.staging[name] = tensor.clone() if tensor.is_cuda else tensor.clone().cuda()
        if poison is not None:
            self.poison[name] = poison
        if inout:
            self.inout.append(name)
        return tensor

    def inp(self, name, value, inout=False, poison=None, pinned=False):
        """A new live buffer whose true value is `value` (any device); pinned: the live buffer is pinned host memory."""
        value = value.detach()
        self.staging[name] = value.cuda().contiguous().clone()
        self.live[name] = (torch.empty(value.shape, dtype=value.dtype).pin_memory() if pinned else torch.empty_like(self.staging[name]))
        if poison is not None:
            self.poison[name] = poison
        if inout:
            self.inout.append(name)
        return self.live[name]

    def outp(self, name, *shape, dtype=torch.float32):
        self.out[name] = torch.empty(*shape, dtype=dtype, device="cuda")
        return self.out[name]

    def __getitem__(self, name):
        return self.live[name] if name in self.live else self.out[name]


def _fill_poison(t, value=None):
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif value is not None:
        t.fill_(value)
    else:
        t.reshape(-1).view(torch.uint8).fill_(POISON_BYTE)


def poison_inputs(b):
    for name, t in b.live.items():
        assert t.dtype.is_floating_point or name in b.poison, f"integer input {name!r} needs a valid poison value"
        _fill_poison(t, b.poison.get(name))


def poison_outputs(b):
    for t in b.out.values():
        _fill_poison(t)


def stage(b):
    for name, t in b.live.items():
        t.copy_(b.staging[name], non_blocking=True)


def read_out(b):
    res = {k: t.clone() for k, t in b.out.items()}
    res.update({k: b.live[k].clone() for k in b.inout})
    return res


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class Case:
    """name; covers: the C-ABI entry points the case calls; make() -> Bufs (fresh model, context and buffers, on the current
    stream); run(bufs): the library calls, on the current stream (returns None, or the stream the results are ordered on);
    reset(bufs): host-only, after the warm-up; sync_free: a host wait inside the calls is a defect, not a short delay."""

    def __init__(self, name, covers, make, run, dtype="f32", reset=None, sync_free=True, delay_ms=DELAY_MS, reads_back=None, warmups=1):
        self.name, self.covers, self.make, self.run, self.dtype = name, tuple(covers), make, run, dtype
        self.warmups = warmups         # (the Python layer has first-use work in an object's SECOND call too: two warm-up passes there)
        self.reset, self.sync_free, self.delay_ms = reset, sync_free, delay_ms
        # a Python-level case that reads back by design (the reason).  One that sets Bufs.checkpoint in front of its closing read
        # is held to `pending` there; one that reads back throughout has only its results compared
        self.reads_back = reads_back

    def __repr__(self):
        return self.name


# ---- the delay ---------------------------------------------------------------------------------------------------------------
_delay = {}


def _delay_state():
    """4096 x 4096 f32 operands and the time of one torch.mm on them, measured once per session with events."""
    if not _delay:
        w = torch.eye(4096, device="cuda")
        a, c = torch.eye(4096, device="cuda"), torch.empty(4096, 4096, device="cuda")
        for _ in range(4):
            torch.mm(a, w, out=c); torch.mm(c, w, out=a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            torch.mm(a, w, out=c); torch.mm(c, w, out=a)
        e1.record()
        torch.cuda.synchronize()
        _delay.update(w=w, a=a, c=c, mm_ms=e0.elapsed_time(e1) / 8)
    return _delay


def chain_length(ms):
    """Products in a chain meant to last `ms` (a quarter more than the measured time asks for, against clock changes; the
    bound on a chain is on what is asked for)."""
    d = _delay_state()
    assert ms <= MAX_DELAY_MS, f"a chain of {ms} ms is above the {MAX_DELAY_MS} ms bound"
    return max(2, math.ceil(1.25 * ms / d["mm_ms"]))


def enqueue_delay(n):
    """n dependent products on the current stream, between two timing events; returns (start, marker)."""
    d = _delay_state()
    start, marker = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    a, c = d["a"], d["c"]
    for _ in range(n):
        torch.mm(a, d["w"], out=c)
        a, c = c, a
    marker.record()
    return start, marker


# ---- the two runs ------------------------------------------------------------------------------------------------------------
def reference_run(case):
    """Default stream, fresh model and context, a device synchronisation on either side of the calls."""
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    b = case.make()
    poison_outputs(b)
    stage(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    case.run(b)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    res = read_out(b)
    torch.cuda.synchronize()
    return res, host_ms


def stream_run(case, delay_ms=DELAY_MS):
    """The same calls on the non-default stream the control has proven (case_stream), enqueued while that stream is held up.
    Returns (results, info)."""
    s = case_stream()
    n = chain_length(delay_ms)
    with torch.cuda.stream(s):
        b = case.make()
        for _ in range(case.warmups):
            stage(b)                               # 1. warm-up with the true inputs
            warm = case.run(b)
            enqueue_delay(2)
            s.synchronize()
            if warm is not None:
                warm.synchronize()                 # (a two-stream case: its second stream is idle too before anything is poisoned)
        if case.reset is not None:
            case.reset(b)                          # host-side counters of the Python layer back to a fresh object's
        poison_inputs(b)                           # 2. poison
        poison_outputs(b)
        s.synchronize()
        gc.collect()                               # (a collector pause of tens of ms is not a wait inside the library:
        gc.disable()                               #  none while the host enqueues against the chain)
        try:
            start, marker = enqueue_delay(n)       # 3. delay
            t0 = time.perf_counter()
            poison_outputs(b)                      # 4. (the outputs once more, in stream order: a result written early is lost)
            stage(b)
            b.probe = lambda: not marker.query()
            last = case.run(b)
            last = s if last is None else last     # (a two-stream case names the stream its results are ordered on)
            with torch.cuda.stream(last):
                res = read_out(b)
            pending = not marker.query()           # 5.
            if b.checkpoint is not None:           # (a case that closes with a read-back by design: what it saw in front of it)
                pending = b.checkpoint
            host_ms = (time.perf_counter() - t0) * 1e3
        finally:
            gc.enable()
        last.synchronize()                         # 6. the only synchronisation
    chain_ms = start.elapsed_time(marker)
    torch.cuda.synchronize()                       # (after the comparison data is safe: nothing of this case outlives it)
    return res, dict(pending=pending, checked=b.checkpoint is not None, host_ms=host_ms, chain=n, chain_ms=chain_ms)


def check_case(case, exempt=None):
    """Run `case` both ways and compare.  Returns the record line; raises AssertionError on any violation."""
    ref, host1 = reference_run(case)
    ref2, host2 = reference_run(case)
    delay_ms = case.delay_ms
    if not case.sync_free:      # a Python-level case: its own figure, a multiple of its host time on the idle default stream
        delay_ms = min(MAX_DELAY_MS, max(delay_ms, PYTHON_DELAY_FACTOR * min(host1, host2)))
    got, info = stream_run(case, delay_ms)
    info["ref_host_ms"] = min(host1, host2)
    gated, wrong = [], []
    for name in ref:
        if same_bits(ref[name], ref2[name]):
            if not same_bits(got[name], ref[name]):
                wrong.append(f"{name}: bits differ from the default-stream run")
        else:                                      # two default-stream runs disagree (f64 atomics): the parity gate instead
            gate, err, spread = GATE[case.dtype], rel_l2(got[name], ref[name]), rel_l2(ref2[name], ref[name])
            gated.append(f"{name} ({err:.2e}, default-stream spread {spread:.2e})")
            if not err <= gate:
                wrong.append(f"{name}: relative L2 {err:.3e} above the gate {gate:g}")
    rec = dict(case=case.name, how="gate: " + ", ".join(gated) if gated else "bits", wrong=wrong, **info)
    RECORD.append(rec)
    line = (f"{case.name}: host {info['host_ms']:.2f} ms (idle default stream {info['ref_host_ms']:.2f} ms), chain {info['chain']} x mm = {info['chain_ms']:.1f} ms, pending {info['pending']}, "
            f"{rec['how']}" + ("".join("; " + w for w in wrong)))
    print(line)
    assert info["chain_ms"] >= DELAY_MS, f"the delay lasted {info['chain_ms']:.1f} ms, under {DELAY_MS} ms: {line}"
    results_only = case.reads_back and not info["checked"]      # reads back throughout: only its results are compared
    if not info["pending"] and not (exempt and case.name in exempt) and not results_only:
        raise AssertionError(("the host waited inside the library: " if case.sync_free else "inconclusive, the delay was too short: ") + line)
    assert not wrong, line
    return rec


_case_stream = {}


def case_stream():
    """The stream every case runs on: the first of up to 8 new streams on which the control sees the poison.  HIP maps its
    streams onto a few hardware queues (GPU_MAX_HW_QUEUES); a stream that shares its queue with the default stream runs in
    order with it, a launch that strayed to stream 0 would look right there, and the control says so.  Such a stream is no
    use as a witness, so the harness takes one that the control has shown to be independent - and fails if there is none."""
    if "s" not in _case_stream:
        _case_stream["tried"] = []
        for _ in range(8):
            s = torch.cuda.Stream()
            c = control(s)
            _case_stream["tried"].append(c)
            if c["pending"] and c["all_poison"] and c["settled"]:
                _case_stream["s"] = s
                break
    assert "s" in _case_stream, f"the control saw the true values on every stream tried: the harness is blind: {_case_stream['tried']}"
    return _case_stream["s"]


def control(s):
    """A plain torch op on the default stream racing a copy on the delayed stream `s`: it must see the poison."""
    truth = torch.rand(1 << 16, device="cuda")
    live = torch.empty_like(truth)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        enqueue_delay(2)
        s.synchronize()
        live.fill_(float("nan"))
        s.synchronize()
        start, marker = enqueue_delay(chain_length(DELAY_MS))
        live.copy_(truth, non_blocking=True)
    y = live * 2                                    # default stream, outside the block: not ordered behind s
    torch.cuda.default_stream().synchronize()
    pending = not marker.query()
    torch.cuda.synchronize()
    return dict(pending=pending, saw_poison=bool(torch.isnan(y).any()), all_poison=bool(torch.isnan(y).all()),
                chain_ms=start.elapsed_time(marker), settled=same_bits(live, truth))


def write_record(path, header=()):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for h in header:
            f.write(h + "\n")
        f.write(f"one torch.mm 4096x4096 f32: {_delay_state()['mm_ms']:.3f} ms\n")
        for i, c in enumerate(_case_stream.get("tried", [])):
            f.write(f"control on stream {i + 1} tried: {c}\n")
        f.write("case | host enqueue ms | chain (products, ms) | pending | compared by | found\n")
        for r in RECORD:
            f.write(f"{r['case']} | {r['host_ms']:.2f} (idle {r['ref_host_ms']:.2f}) | {r['chain']}, {r['chain_ms']:.1f} | {r['pending']} | {r['how']} | "
                    f"{'; '.join(r['wrong']) or '-'}\n")
