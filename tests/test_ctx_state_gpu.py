"""Which forward a context holds, and what it lets follow: the host-side refusals of the C ABI (include/vae_step.h) that depend
on the last forward, through a model's context handle.  Every expected failure is a refusal on the host, nothing provokes a device fault.  Reference-exact model
(32x32, latent 16, batch 4), the smallest shape every path accepts."""
import pytest
import torch

from oracle import vae_oracle as vo
from tests.util import make_model, perturbed_params
from torch_vae_amd import _lib

pytestmark = pytest.mark.gpu

H, L, B = 32, 16, 4


class Ctx:
    """A model's context handle with caller-owned tensors of one batch; every method returns the entry point's return code."""

    def __init__(self, dtype="bf16"):
        self.m = m = make_model(H, L, False, dtype, perturbed_params(L, H, 31, False))
        self.lib = _lib.lib()
        self.h = m._context(B).handle                       # a context with no forward
        self.st = torch.cuda.current_stream().cuda_stream
        self.x = torch.from_numpy(vo.synth_pianoroll(B, H, 32)).float().cuda()
        self.xhat = torch.empty_like(self.x)
        self.mu, self.lv, self.z, self.g_lat = (torch.zeros(B, L, device="cuda") for _ in range(4))
        self.out3 = torch.empty(3, device="cuda")
        self.big = torch.empty(B * 32 * 16 * 16, device="cuda")     # the largest debug tensor asked for (y of encoder.0)
        self.kl = torch.empty(L, device="cuda", dtype=torch.float64)
        self.one = torch.ones(1, device="cuda")
        self.dx = torch.empty_like(self.x)
        self.dz = torch.empty(B, L, device="cuda")

    def err(self):
        return self.lib.vae_last_error().decode()

    def forward(self, train, batch=B, seed=7, running=True):
        m = self.m
        return self.lib.vae_forward(self.h, self.x.data_ptr(), batch, m._flat.data_ptr(), m._bnflat.data_ptr() if running else 0, m._nbt.data_ptr(), 0, seed,
                                    train, self.xhat.data_ptr(), self.mu.data_ptr(), self.lv.data_ptr(), self.z.data_ptr(), self.st)

    def encode(self, train=1, running=True):
        m = self.m
        return self.lib.vae_encode(self.h, self.x.data_ptr(), B, m._flat.data_ptr(), m._bnflat.data_ptr() if running else 0, m._nbt.data_ptr(), 0, 7, train,
                                   self.mu.data_ptr(), self.lv.data_ptr(), self.z.data_ptr(), self.st)

    def decode(self, train=1, running=True):
        m = self.m
        return self.lib.vae_decode(self.h, self.z.data_ptr(), B, m._flat.data_ptr(), m._bnflat.data_ptr() if running else 0, m._nbt.data_ptr(), train,
                                   self.xhat.data_ptr(), self.st)

    def log_likelihood(self):
        m = self.m
        lw, ll, elbo = (torch.empty(n, device="cuda", dtype=torch.float64) for n in (2 * B, B, B))
        return self.lib.vae_log_likelihood(self.h, self.x.data_ptr(), B, m._flat.data_ptr(), m._bnflat.data_ptr(), 2, 1, 0, 9,
                                           lw.data_ptr(), ll.data_ptr(), elbo.data_ptr(), self.st)

    def loss(self):
        return self.lib.vae_loss(self.h, 1.0, self.out3.data_ptr(), self.st)

    def loss_bits(self):
        assert self.loss() == 0, self.err()
        torch.cuda.synchronize()
        return self.out3.clone()

    def loss_deferred(self):
        return self.lib.vae_loss_deferred(self.h, 1.0, self.out3.data_ptr(), self.st)

    def pre_latents(self):
        return self.lib.vae_pre_latents(self.h, self.big.data_ptr(), self.st)

    def last_eps(self):
        return self.lib.vae_last_eps(self.h, self.big.data_ptr(), self.st)

    def debug_tensor(self):
        return self.lib.vae_debug_tensor(self.h, 0, self.big.data_ptr(), self.big.numel(), self.st)

    def kl_per_dim(self):
        return self.lib.vae_kl_per_dim(self.h, self.kl.data_ptr(), self.st)

    def backward(self, gscale=None, part=None, use_std=1):
        m = self.m
        args = (self.h, self.x.data_ptr(), m._flat.data_ptr(), m._gflat.data_ptr(), 0, _lib.ptr(gscale), 0, 0, 0, 0, 1.0, use_std)
        if part is None:
            return self.lib.vae_backward(*args, self.st)
        return self.lib.vae_backward_part(*args, part, self.st)

    def backward_ex(self, use_std=0, g_mu=None, dz=None):
        m = self.m
        return self.lib.vae_backward_ex(self.h, self.x.data_ptr(), m._flat.data_ptr(), m._gflat.data_ptr(), 0, 0, _lib.ptr(g_mu), 0, 0, 0,
                                        1.0, use_std, 0, _lib.ptr(dz), self.st)


def refused(c, rc, message):
    assert rc == -1 and message in c.err(), (rc, c.err(), message)


def succeeds(c, rc):
    assert rc == 0, c.err()
    torch.cuda.synchronize()


def test_fresh_context_holds_no_forward():
    c = Ctx()
    refused(c, c.loss(), "no forward")
    refused(c, c.loss_deferred(), "no forward")
    refused(c, c.pre_latents(), "no forward")
    refused(c, c.last_eps(), "no forward")
    refused(c, c.debug_tensor(), "no forward")
    refused(c, c.kl_per_dim(), "no forward with a posterior")
    refused(c, c.backward(), "no train-mode forward")
    refused(c, c.backward_ex(use_std=1), "no forward to differentiate")


def test_after_encode():
    c = Ctx()
    succeeds(c, c.encode())
    refused(c, c.backward(), "use vae_backward_ex")
    refused(c, c.backward_ex(use_std=1), "encode-only")
    refused(c, c.backward_ex(dz=c.dz), "decode-only forward")
    refused(c, c.loss_deferred(), "train-mode forward")
    succeeds(c, c.kl_per_dim())


def test_after_decode():
    c = Ctx()
    succeeds(c, c.decode())
    refused(c, c.backward(), "use vae_backward_ex")
    refused(c, c.backward_ex(use_std=1), "decode-only")
    refused(c, c.backward_ex(g_mu=c.g_lat), "only g_xhat and dz apply")
    refused(c, c.kl_per_dim(), "no forward with a posterior")


def test_after_eval_forward():
    c = Ctx()
    succeeds(c, c.forward(train=0))
    refused(c, c.backward(), "no train-mode forward")
    refused(c, c.loss_deferred(), "train-mode forward")
    succeeds(c, c.loss())
    succeeds(c, c.backward_ex(use_std=1))


def test_backward_parts_after_train_forward():
    c = Ctx()
    succeeds(c, c.forward(train=1))
    refused(c, c.backward(part=2), "part 2 before part 1")
    refused(c, c.backward(part=3), "part must be")


def test_deferred_output_conv_bf16():
    c = Ctx("bf16")
    succeeds(c, c.forward(train=2))
    refused(c, c.loss(), "train = 2")
    refused(c, c.backward(gscale=c.one), "only the standard ELBO backward")
    succeeds(c, c.backward())
    refused(c, c.backward(), "already consumed")


def test_output_conv_not_deferred_f32():
    c = Ctx("f32")
    succeeds(c, c.forward(train=2))
    succeeds(c, c.loss())


def test_log_likelihood_leaves_no_forward():
    c = Ctx()
    succeeds(c, c.forward(train=1))
    succeeds(c, c.log_likelihood())
    refused(c, c.loss(), "no forward")
    refused(c, c.backward(), "no train-mode forward")
    refused(c, c.backward_ex(use_std=1), "no forward to differentiate")


def test_oversize_batch_leaves_the_previous_forward():
    c = Ctx()
    succeeds(c, c.forward(train=1))
    before = c.loss_bits()
    refused(c, c.forward(train=1, batch=c.m._ctx.key[2] + 1), "max_batch")
    assert torch.equal(c.loss_bits(), before)


def test_settings_are_recorded_per_forward():
    c = Ctx()
    succeeds(c, c.forward(train=1))
    before = c.loss_bits()
    assert c.lib.vae_set_recon_loss(c.h, _lib.RECON_MSE) == 0 and c.lib.vae_set_kl_objective(c.h, _lib.KL_FREE_BITS, 0.5) == 0
    assert torch.equal(c.loss_bits(), before)
    succeeds(c, c.forward(train=1))
    assert not torch.equal(c.loss_bits(), before)


@pytest.mark.parametrize("entry", ["forward", "encode", "decode"])
def test_forward_refused_half_way_leaves_no_forward(entry):
    """An eval-mode pass without running statistics is refused on the host INSIDE the implementation, after its first launches
    (a refusal, not a fault).  The forward held before it is gone, and so is the half-finished one."""
    c = Ctx()
    succeeds(c, c.forward(train=1))
    succeeds(c, c.loss())
    refused(c, getattr(c, entry)(train=0, running=False), "eval mode needs running statistics")
    torch.cuda.synchronize()
    refused(c, c.loss(), "no forward")
    refused(c, c.pre_latents(), "no forward")
    refused(c, c.backward(), "no train-mode forward")
    refused(c, c.backward_ex(use_std=0), "no forward to differentiate")
    succeeds(c, c.forward(train=1))          # and the context is usable again
    succeeds(c, c.loss())


def test_a_new_forward_starts_a_new_backward():
    c = Ctx()
    succeeds(c, c.forward(train=1))
    succeeds(c, c.backward(part=1))
    succeeds(c, c.forward(train=1))
    refused(c, c.backward(part=2), "part 2 before part 1")
    succeeds(c, c.backward(part=1))
    succeeds(c, c.backward(part=2))
