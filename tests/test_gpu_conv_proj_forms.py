"""The message kernel of the basis form (conv_proj.hip) at the smallest sizes where its slot sequence can go wrong.

One ragged batch of 13 crystals, 300 receivers: more than the 240 from which ARREAU_BASIS_MIN_RECEIVERS=240 selects the basis
form, not a multiple of the grid (one persistent workgroup per CU: on a 256-CU part 44 workgroups walk two receivers, the
others one, i.e. the last round has fewer receivers than CUs), graph teacher-forced with every degree from 0 to 8 (degree 0: only
zero blocks; 1, 7 and 8: the odd / even ends of a receiver's eight slots).  Everything goes through the ctypes API.

Which comparison is bitwise: internal.h documents the basis form with THREE fp16 products (ARREAU_CROSS_FP8=0) as bit-identical
to the K pair; the default form runs the two cross products on the fp8 matrix instruction and is documented (and asserted in
test_gpu_parity.py) as close to it, not equal.  So `torch.equal` against the K pair is asserted for the fp16-cross form, the
default form is held against it to the share of the parity bounds that the product itself grants the fp8 formats, and the
properties that need no second path (unused slots, eager against graph replay) are asserted bitwise on the default form.
"""
import os

import pytest
import torch

from tests.helpers import TOL, pooled_bound, random_state

pytestmark = pytest.mark.gpu

COUNTS = [24, 23, 25, 22, 26, 21, 27, 20, 28, 19, 29, 18, 18]  # 300 receivers = 256 + 44
T_EVAL = 400


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(dev):
    from arreau_amd.checkpoint import make_synthetic_model
    return make_synthetic_model(S=90, seed=1234).to(dev)


class _Env:
    """Environment switches the library reads per call, restored on exit."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


K_PAIR = dict(ARREAU_BASIS_MIN_RECEIVERS=None, ARREAU_CROSS_FP8=None)
BASIS_FP16_CROSS = dict(ARREAU_BASIS_MIN_RECEIVERS="240", ARREAU_CROSS_FP8="0")
BASIS_DEFAULT = dict(ARREAU_BASIS_MIN_RECEIVERS="240", ARREAU_CROSS_FP8=None)


@pytest.fixture(scope="module")
def batch(dev, model):
    """The batch, its teacher-forced graph (the kernel's own neighbour list cut to degrees 0, 1, .., 8, 0, 1, ..) and the K pair's
    outputs on it: computed once, shared, never modified."""
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    eng = model.engine()
    frac, types, lengths, angles, na = random_state(90, COUNTS, 41, cell=(4.0, 8.0))
    N, B = sum(COUNTS), len(COUNTS)
    assert B == 13 and N >= 241 and N % 256 != 0 and N < 2 * 256
    d = lambda v: v.to(dev).contiguous()
    args = (d(frac), d(types.to(torch.int32)), d(lengths), d(angles), torch.full((B,), T_EVAL, device=dev, dtype=torch.int32),
            crystal_offsets(na, dev))
    with _Env(**K_PAIR):
        own = eng.predict_scores(*args, return_edges=True)[3]
        deg, src, sdir, sdist = (x.clone() for x in own)
        deg = torch.minimum(deg, (torch.arange(N, device=dev) % 9).to(torch.int32))
        have = set(deg.tolist())
        assert {0, 1, 7, 8} <= have and have == set(range(9)), have
        edges = (deg, src, sdir, sdist)
        ref = eng.predict_scores(*args, edges=edges)
        assert eng.check_status()["conv_variant"] == 1  # the K pair really ran
    return {"args": args, "edges": edges, "ref": tuple(x.clone() for x in ref), "N": N, "B": B}


def _basis_scores(eng, batch, env, edges=None):
    with _Env(**env):
        out = eng.predict_scores(*batch["args"], edges=edges or batch["edges"])
        st = eng.check_status()
    assert st["conv_variant"] == 2, st  # conv_proj_kernel really ran
    assert st["conv_cross_fp8"] == (0 if env.get("ARREAU_CROSS_FP8") == "0" else 1), st
    return out


def test_basis_form_is_bitwise_the_k_pair_on_the_ragged_batch(dev, model, batch):
    """Degrees 0..8, 300 receivers on a grid of one workgroup per CU: the basis form with three fp16 products against the K pair,
    eps, logits and len0 bit for bit (the identity internal.h documents for ARREAU_CROSS_FP8=0)."""
    got = _basis_scores(model.engine(), batch, BASIS_FP16_CROSS)
    for name, a, b in zip(("eps", "logits", "len0"), got, batch["ref"]):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def test_default_form_stays_within_its_calibration_share_of_the_k_pair(dev, model, batch):
    """The default form (cross products on the fp8 matrix instruction) is documented as NOT bit-identical to the K pair.  The bound
    is the one the product applies when it accepts the format for a model (model.hip, calibrate_message_formats): the outputs may
    move by at most a tenth of their parity bounds, 1e-6 max(1, |eps|) and 1e-6 max(1, |logits| / 8); len0, a per-crystal sum, a
    tenth of tests.helpers.pooled_bound."""
    got = _basis_scores(model.engine(), batch, BASIS_DEFAULT)
    ref = batch["ref"]
    e, l, g = (float((a - b).abs().max()) for a, b in zip(got, ref))
    print(f"[conv_proj forms] |fp8 cross - K pair| : eps {e:.2e}  logits {l:.2e} (|logits| {float(ref[1].abs().max()):.1f})"
          f"  len0 {g:.2e} (|len0| {float(ref[2].abs().max()):.1f})")
    share = 0.1  # ARREAU_CALIB_SHARE
    assert e <= share * TOL * max(1.0, float(ref[0].abs().max()))
    assert l <= share * TOL * max(1.0, float(ref[1].abs().max()) / 8.0)
    assert g <= share * pooled_bound(ref[2].cpu(), atoms_per_crystal=max(COUNTS))


@pytest.mark.parametrize("env", [BASIS_DEFAULT, BASIS_FP16_CROSS], ids=["fp8 cross (default)", "fp16 cross"])
def test_unused_slots_are_not_inputs(dev, model, batch, env):
    """Slots past a receiver's degree filled with NaN, infinities and a huge value (include/arreau_hip.h: they are not inputs): the
    outputs do not move by a bit, for every degree from 0 to 8."""
    eng = model.engine()
    deg, src, sdir, sdist = batch["edges"]
    want = tuple(x.clone() for x in _basis_scores(eng, batch, env))
    unused = torch.arange(8, device=dev)[None, :] >= deg[:, None]
    for fill in (float("nan"), float("inf"), -3.0e38):
        sdir_f, sdist_f, src_f = sdir.clone(), sdist.clone(), src.clone()
        sdir_f[unused] = fill
        sdist_f[unused] = fill
        src_f[unused] = 0
        got = _basis_scores(eng, batch, env, edges=(deg, src_f, sdir_f, sdist_f))
        for a, b in zip(got, want):
            assert torch.equal(a, b), fill
    for x in want:
        assert torch.isfinite(x).all()


def test_eager_loop_is_bitwise_graph_replay_on_the_ragged_batch(dev, model, batch):
    """Three steps of the sampling loop on the same 300-receiver batch with the basis form: eager launches and the replayed graph
    hand back the same bits."""
    eng = model.engine()
    B, off = batch["B"], batch["args"][5]
    # (the same crystals, drawn like the sampler's start: the loop takes monoclinic angles in degrees)
    d = lambda v: v.to(dev).contiguous()
    frac, types, lengths, angles = (d(x) for x in random_state(90, COUNTS, 43, sampler_like=True)[:4])
    types = types.to(torch.int32)

    def loop(use_graph):
        f, ty, le, lat = frac.clone(), types.clone(), lengths.clone(), torch.zeros(B, 3, 3, device=dev)
        eng.sample_loop(f, ty, le, angles, off, 999, 3, 4242, None, lat, use_graph=use_graph)
        return f, ty, le, lat

    with _Env(**BASIS_DEFAULT):
        ref = loop(False)
        assert eng.check_status()["conv_variant"] == 2
        got = loop(True)
        eng.check_status()
    for x, y in zip(ref, got):
        assert torch.equal(x, y)
