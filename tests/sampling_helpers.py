"""Shared scaffolding of the sampling GPU tests (test_gpu_{respaced,conditioned,corrector,resampled}_sampling.py): the synthetic
models, a ragged sampler state on the device and the comparisons.  A test module imports the fixtures `dev`, `model_seed`,
`fused_model` and `any_model` by name (a module may define its own `model_seed` instead) and subclasses Case with its COUNTS."""
import numpy as np
import pytest
import torch

from tests.helpers import oracle_from_module, random_state

S, T = 12, 100  # the synthetic models' species and timesteps


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model_seed():
    return 4321


def _model(dev, kind, seed):
    from arreau_amd.checkpoint import make_synthetic_model
    shape = {} if kind == "fused" else dict(hidden_dim=64, basis_dim=96, widening_factor=2, layers=3)
    m = make_synthetic_model(S=S, seed=seed, num_timesteps=T, **shape).to(dev)
    return m, oracle_from_module(m, torch.float32)


@pytest.fixture(scope="module")
def fused_model(dev, model_seed):
    return _model(dev, "fused", model_seed)


@pytest.fixture(scope="module", params=["fused", "general-C64"])
def any_model(dev, request, fused_model, model_seed):
    return fused_model if request.param == "fused" else _model(dev, request.param, model_seed)


class Case:
    """A ragged sampler state (tests.helpers.random_state) with its CSR offsets and angles on the device; `counts` defaults
    to the subclass's COUNTS."""
    COUNTS = None

    def __init__(self, dev, seed=5, counts=None, sampler_like=True):
        counts = self.COUNTS if counts is None else counts
        self.frac, self.types, self.lengths, self.angles, self.na = random_state(S, counts, seed, sampler_like=sampler_like)
        from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
        self.B, self.N, self.dev = len(counts), sum(counts), dev
        self.off = crystal_offsets(self.na, dev)
        self.an = self.angles.to(dev).contiguous()
        self.crystal = np.repeat(np.arange(self.B), counts)

    def fresh(self):
        d = lambda v: v.to(self.dev).contiguous()
        return (d(self.frac.clone()), d(self.types.to(torch.int32)), d(self.lengths.clone()),
                torch.zeros(self.B, 3, 3, device=self.dev))

    def load(self, bufs):
        """The initial state into existing buffers (a graph is cached for the buffers it was captured on)."""
        for a, b in zip(bufs, self.fresh()):
            a.copy_(b)
        return bufs


def full_i32(n, v, dev):
    return torch.full((n,), v, device=dev, dtype=torch.int32)


def wrapped_dist(a, b):
    """Elementwise distance of fractional coordinates on the unit circle, in float64."""
    dd = (a.double() - b.double()).abs()
    return torch.minimum(dd, 1 - dd)


def assert_same_bits(got, want, what, nan_ok=False):
    """Pairwise the same dtype, shape and bytes, and no NaN in a float tensor (bit-equal NaNs would pass the byte test).
    nan_ok: NaNs in the same bits pass (a state that overflowed the fp16x3 kernels the same way in both runs)."""
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert nan_ok or not (a.is_floating_point() and bool(torch.isnan(a).any())), what
        assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)), what
