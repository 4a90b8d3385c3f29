"""numpy float64 restatement of the weight averaging (include/vae_average.h): the weight rule, the lerp and the gate.  The tests
compare the HIP kernels and the Python layer against it; tests/test_average_host.py pins it against
torch.optim.swa_utils.AveragedModel."""
import numpy as np

EMA, EQUAL = 0, 1
KINDS = {"ema": EMA, "swa": EQUAL}


def weight(kind, n, decay=0.999, warmup=0.0):
    """(copy, w) of the update that finds ``n`` updates applied: w in float64, before its one rounding to float32."""
    if n == 0:
        return True, 1.0
    if kind == EQUAL:
        return False, 1.0 / (float(n) + 1.0)
    d = float(decay)
    if warmup > 0.0:
        d = min(d, (1.0 + float(n)) / (float(warmup) + float(n)))
    return False, 1.0 - d


def weight_f32(kind, n, decay=0.999, warmup=0.0) -> float:
    """The weight as the kernel applies it and reports it in last_weight: rounded once to float32."""
    return float(np.float32(weight(kind, n, decay, warmup)[1]))


def lerp(e, s, w, copy=False):
    """avg' of one update in float64: s for the copy, else e + w (s - e)."""
    s = np.asarray(s, np.float64)
    if copy:
        return s.copy()
    e = np.asarray(e, np.float64)
    return e + w * (s - e)


class AverageRef:
    """The device state and the averaged segments of vae_average_update, in float64."""

    def __init__(self, kind, decay=0.999, warmup=0.0, seen_step=-1, n_averaged=0):
        self.kind = KINDS.get(kind, kind)
        self.decay, self.warmup = decay, warmup
        self.seen_step, self.n_averaged, self.last_weight = seen_step, n_averaged, 0.0
        self.avg = None

    def update(self, srcs, opt_step=None, scales=None) -> bool:
        """One call on the segments ``srcs``; returns whether the gate let it apply."""
        if opt_step is not None and opt_step == self.seen_step:
            return False
        copy, w = weight(self.kind, self.n_averaged, self.decay, self.warmup)
        scales = [1.0] * len(srcs) if scales is None else scales
        # (the kernel forms s = src * scale in float32; for a scale of 1 that is src itself)
        s = [np.asarray(x, np.float64) if c == 1.0 else (np.asarray(x, np.float32) * np.float32(c)).astype(np.float64) for x, c in zip(srcs, scales)]
        old = s if self.avg is None else self.avg
        self.avg = [lerp(e, x, w, copy) for e, x in zip(old, s)]
        if opt_step is not None:
            self.seen_step = opt_step
        self.n_averaged += 1
        self.last_weight = float(np.float32(w))
        return True


def recovered_bn_stat(running_after):
    """The batch statistic a train-mode forward from ZEROED buffers left as fl(0.1f * stat): 10 * running', in float32 as the kernel
    forms it (update_bn)."""
    return (np.asarray(running_after, np.float32) * np.float32(10.0)).astype(np.float64)
