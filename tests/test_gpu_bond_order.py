"""Bond angles and Steinhardt order parameters on the device (arreau_crystal_bond_order, csrc/bond_order.hip) on the cases of
tests/bond_order_cases.py: against the float32 restatement bit for bit on every case (integers equal, floats equal as bits, NaN
patterns included), a crystal alone against the same crystal inside its batch, from_coordination against the chain,
Engine.bond_order, sample(bond_order=...), the two command lines, the argument errors and the export.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import bond_order as bo
from arreau_amd.diffusion import coordination as co
from tests import bond_order_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["shells", "full", "random", "bad_list", "known", "known tol0", "skewed", "flags", "overflow", "large", "ragged"]
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, case):
    off = np.concatenate([[0], np.cumsum(case.counts)]).astype(np.int32)
    return up(dev, case.frac.reshape(-1, 3)), up(dev, case.lattice), up(dev, off)


def launch(dev, case):
    """The kernel's arrays of a case: the chain (device coordination search, then the new launch), or the new launch alone on the
    uploaded lists where they are hand-made."""
    if case.handmade:
        lists = {"cn": up(dev, case.cn), "neighbors": up(dev, case.neighbors)}
        return bo.result_to_numpy(bo.from_coordination(*device_batch(dev, case), lists))
    return bo.result_to_numpy(bo.bond_order(*device_batch(dev, case), case.params))


def run(dev, name):
    if name not in _RUN:
        _RUN[name] = launch(dev, cases.references()[name][0])
    return _RUN[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k] if isinstance(want, dict) else getattr(want, k))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, k, np.flatnonzero((bits(g) != bits(w)).reshape(len(w), -1).any(axis=1))[:8])


def test_the_case_list_is_what_the_tests_name():
    assert list(cases.references()) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_float32_restatement_bit_for_bit(dev, name):
    case, r32, _ = cases.references()[name]
    got = run(dev, name)
    assert set(got) == set(bo.RESULT_KEYS) | (set() if case.handmade else {"coord_flags"})
    same(got, r32, bo.RESULT_KEYS, name)
    if not case.handmade:
        assert np.array_equal(got["coord_flags"], case.coord_flags)


def test_sizes_and_flags_on_the_device(dev):
    full, case = run(dev, "full"), cases.references()["full"][0]
    assert full["n_used"][:2].tolist() == [64, 64] and full["angles"][:2].sum(axis=1).tolist() == [2016, 2016]
    assert full["flags"][:2].tolist() == [0, bo.TRUNCATED] and case.cn[1] == 78
    assert run(dev, "bad_list")["flags"].tolist() == [0, bo.BAD_LIST, bo.BAD_LIST, 0]
    assert run(dev, "shells")["flags"].tolist() == [0, 0, bo.ISOLATED, 0, 0, 0, bo.OVERLAP]
    large, lc = run(dev, "large"), cases.references()["large"][0]
    assert lc.counts[1] == co.cb.STAGED_ATOMS + 3 and (large["flags"] == 0).all() and np.isfinite(large["q"]).all()
    # no crystals at all: nothing is launched
    empty = bo.bond_order(torch.empty((0, 3), device=dev), torch.empty((0, 3, 3), device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
    assert empty["flags"].shape == (0,) and empty["angles"].shape == (0, 37) and empty["mean_q"].shape == (0, 4)


def test_a_crystal_alone_gives_the_bits_it_gives_in_the_batch(dev):
    for name, picks in (("ragged", (33, 0, 69)), ("large", (1,)), ("full", (0, 1)), ("bad_list", (1, 3))):
        case = cases.references()[name][0]
        got = run(dev, name)
        first = cases.first_atoms(case)
        for b in picks:
            alone = launch(dev, cases.single(case, b))
            for k in bo.CRYSTAL_KEYS:
                assert np.array_equal(bits(alone[k][0]), bits(got[k][b])), (name, b, k)
            for k in bo.RESULT_KEYS[len(bo.CRYSTAL_KEYS):]:
                assert np.array_equal(bits(alone[k]), bits(got[k][first[b]:first[b + 1]])), (name, b, k)
    again = launch(dev, cases.references()["ragged"][0])  # and a second launch of the whole batch
    same(again, run(dev, "ragged"), bo.RESULT_KEYS, "ragged again")


def test_from_coordination_and_the_engine_equal_the_chain(dev, fused_model):
    case = cases.references()["random"][0]
    frac, lattice, off = device_batch(dev, case)
    found = co.coordination(frac, lattice, off, case.params.coordination())
    direct = bo.result_to_numpy(bo.from_coordination(frac, lattice, off, found, case.params.max_neighbors))
    same(direct, run(dev, "random"), bo.RESULT_KEYS + ("coord_flags",), "from_coordination")
    with pytest.raises(ValueError, match="neighbors"):
        bo.from_coordination(frac, lattice, off, found, 16)  # not the width of the result's lists
    eng = fused_model[0].engine()
    same(bo.result_to_numpy(eng.bond_order(frac, lattice, off, case.params)), direct, bo.RESULT_KEYS + ("coord_flags",), "engine")
    same(bo.result_to_numpy(eng.bond_order(frac, lattice, off, case.params, found)), direct, bo.RESULT_KEYS + ("coord_flags",), "engine, shared search")
    full = cases.references()["full"][0]
    same(bo.result_to_numpy(eng.bond_order(*device_batch(dev, full), full.params)), run(dev, "full"), bo.RESULT_KEYS, "engine, 64 wide")


def test_sample_with_bond_order(dev, fused_model):
    m, _ = fused_model
    params = bo.BondOrderParams(tol=0.15, cutoff=5.0, max_neighbors=16)
    with pytest.raises(ValueError, match="must agree"):  # before any work: the generators are not read
        state = torch.random.get_rng_state()
        m.sample([4, 7, 1], 3, seed=777, max_steps=6, bond_order=params, coordination=True)
    assert torch.equal(state, torch.random.get_rng_state())
    out = []
    for kw in ({}, dict(bond_order=True), dict(bond_order=None), dict(coordination=params.coordination(), screen=True),
               dict(bond_order=params, coordination=params.coordination(), screen=True)):
        torch.manual_seed(3)
        np.random.seed(3)
        r = m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)
        out.append((r, torch.random.get_rng_state(), np.random.uniform()))
    plain = out[0][0]
    for r, rng, after in out[1:]:
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and np.array_equal(plain.num_atoms, r.num_atoms)
        assert torch.equal(out[0][1], rng) and out[0][2] == after
    a, none, without, both = out[1][0], out[2][0], out[3][0], out[4][0]
    assert plain.bond_order is None and none.bond_order is None and without.bond_order is None
    assert a.coordination is None and a.metrics is None and a.symmetry is None
    for field in ("coordination", "metrics"):  # the coordination arrays and the screen's: as without the keyword
        x, y = getattr(both, field), getattr(without, field)
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))), (field, k)
    for r, p in ((a, None), (both, params)):
        c = r.bond_order
        assert tuple(c) == bo.STORED_KEYS and c["q"].shape == (12, 4) and c["angles"].shape == (12, 37) and c["mean_q"].shape == (3, 4)
        assert np.array_equal(c["species"], np.rint(r.atomic_numbers).astype(np.int64))
        same(bo.bond_order_sample_result(r, p, dev), c, bo.STORED_KEYS, "engine-free")
        cn, nb = bo.reference_lists(r.frac_x, r.lattice, r.num_atoms, p)
        same(c, bo.bond_order_reference_f32(r.frac_x, r.lattice, r.num_atoms, cn, nb), bo.RESULT_KEYS, "restatement")
    assert np.array_equal(both.bond_order["coord_flags"], both.coordination["flags"])


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_write_and_print_the_same_numbers(dev, tmp_path):
    """generate --bond_order --coordination, then screen --bond_order --out on the file it wrote: each a fresh process; and the
    screen on a file of the known structures."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out, out2 = str(tmp_path / "out" / "crystals.npz"), str(tmp_path / "again.npz")
    flags = ["--bond_order", "--cn_tol", "0.2", "--cn_cutoff", "5.5"]
    text = _child(["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "10",
                   "--seed", "5", "--out", out, "--coordination"] + flags, 300)
    lines = [ln for ln in text.splitlines() if ln.startswith("bond order ")]
    assert len(lines) == 2 and re.match(r"bond order rank 0: 5 crystals, \d+ atoms; angles ", lines[0]) and lines[1].startswith("bond order total: 5 crystals"), text
    assert len([ln for ln in text.splitlines() if ln.startswith("coordination ")]) == 2 and "screen rank" not in text, text
    res = load_sample_results_from_hdf5(out)
    c = res.bond_order
    assert tuple(c) == bo.STORED_KEYS and c["q"].shape == (30, 4) and np.array_equal(c["coord_flags"], res.coordination["flags"])
    p = bo.BondOrderParams(tol=0.2, cutoff=5.5)
    cn, nb = bo.reference_lists(res.frac_x, res.lattice, res.num_atoms, p)
    same(c, bo.bond_order_reference_f32(res.frac_x, res.lattice, res.num_atoms, cn, nb), bo.RESULT_KEYS, "generate")
    text2 = _child(["arreau_amd.screen", out, "--out", out2] + flags, 120)
    assert [ln for ln in text2.splitlines() if ln.startswith("bond order ")] == lines and "coordination " not in text2, (lines, text2)
    back = load_sample_results_from_hdf5(out2)
    same(back.bond_order, c, bo.STORED_KEYS, "screen")
    same(back.coordination, res.coordination, co.STORED_KEYS, "carried")  # (the file's own coord_* arrays: written again, not recomputed)
    assert back.metrics is not None
    case, r32, _ = cases.references()["known"]
    num = np.array(case.counts, dtype=np.int64)
    known, out3 = str(tmp_path / "known.npz"), str(tmp_path / "known_out.npz")
    save_sample_results_to_hdf5(SampleResult(frac_x=case.frac.astype(np.float64), atomic_numbers=case.species.astype(np.float64),
                                             lattice=case.lattice.astype(np.float64), num_atoms=num, idx_start=np.cumsum(num) - num), known)
    text3 = _child(["arreau_amd.screen", known, "--bond_order", "--out", out3], 120)
    stored = load_sample_results_from_hdf5(out3).bond_order
    same(stored, r32, bo.RESULT_KEYS, "known")
    assert bo.format_stats(bo.total_stats([bo.stats_of(stored)])) in text3 and "Z 29: 0.191 / 0.575" in text3, text3


def test_argument_errors_touch_nothing(dev):
    case = cases.single(cases.references()["known"][0], 5)
    frac, lattice, off = device_batch(dev, case)
    found = co.coordination(frac, lattice, off)
    with pytest.raises(ValueError, match="bond_order: offsets"):
        bo.from_coordination(frac, lattice, off.to(torch.int64), found)
    out = bo.from_coordination(frac, lattice, off, found)
    before = {k: out[k].clone() for k in bo.RESULT_KEYS}
    r = _hip.BondOrderResultC(*[_hip.ptr(out[k]).value for k in bo.RESULT_KEYS])
    edges = [float(e) for e in bo.COS_EDGES]
    params = lambda width=24, e=edges: _hip.BondOrderParamsC(width, (ctypes.c_float * 36)(*e))
    call = _hip.lib().arreau_crystal_bond_order
    EINVAL = -1  # ARREAU_EINVAL
    B, N = 1, int(frac.shape[0])
    cn, nb = _hip.ptr(found["cn"]), _hip.ptr(found["neighbors"])
    swapped, flat, wide, nan = list(edges), list(edges), list(edges), list(edges)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    flat[7] = flat[6]
    wide[0], nan[20] = 1.0, float("nan")
    low = list(edges[:-1]) + [-1.0]
    trials = [(B, N, cn, nb, None, ctypes.byref(r)), (B, N, cn, nb, params(), None), (-1, N, cn, nb, params(), ctypes.byref(r)),
              (B, -1, cn, nb, params(), ctypes.byref(r)), (B, N, None, nb, params(), ctypes.byref(r)), (B, N, cn, None, params(), ctypes.byref(r)),
              (B, N, cn, nb, params(), ctypes.byref(_hip.BondOrderResultC())),
              (B, N, cn, ctypes.c_void_p(nb.value + 4), params(), ctypes.byref(r)),  # neighbours not 16-byte aligned
              (B, N, cn, nb, params(0), ctypes.byref(r)), (B, N, cn, nb, params(65), ctypes.byref(r))]
    trials += [(B, N, cn, nb, params(24, e), ctypes.byref(r)) for e in (swapped, flat, wide, nan, low)]
    for b, n, c_, n_, p, res in trials:
        pp = ctypes.byref(p) if p is not None else None
        assert call(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), b, n, c_, n_, pp, res, _hip.stream_ptr(dev)) == EINVAL, (b, n)
        assert b"arreau_crystal_bond_order" in _hip.lib().arreau_last_error()
    assert call(None, _hip.ptr(lattice), _hip.ptr(off), B, N, cn, nb, ctypes.byref(params()), ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    assert call(None, None, None, 0, 0, None, None, ctypes.byref(params()), ctypes.byref(_hip.BondOrderResultC()), _hip.stream_ptr(dev)) == 0  # B == 0
    torch.cuda.synchronize()
    for k in bo.RESULT_KEYS:
        assert torch.equal(before[k], out[k]), k


def test_sample_takes_the_keyword_and_the_symbol_is_exported(fused_model):
    import inspect
    m, _ = fused_model
    assert "bond_order" in inspect.signature(m.sample).parameters
    assert "arreau_crystal_bond_order" in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_bond_order")
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_bond_order(" in fh.read()
