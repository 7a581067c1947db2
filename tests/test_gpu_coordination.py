"""The coordination search on the device (arreau_crystal_coordination, csrc/coordination.hip) on the batches of
tests/coordination_cases.py: against the float32 restatement bit for bit (integer arrays equal, float arrays equal as bits) on
every case, against the float64 restatement on the guarded crystals (integers equal, distances within the bound derived in
diffusion/screening.py -- never from the kernel's output), a crystal alone against the same crystal inside the 70-crystal batch,
the smallest nearest distance against the screen's min_distance, sample(coordination=...), the two command lines, the argument
errors and the export.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import coordination as co
from arreau_amd.diffusion import screening as sc
from tests import coordination_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["known", "known tol0", "skewed", "flags", "overflow", "large", "ragged"]
INTEGERS = ("n_bonds", "n_mutual", "min_cn", "max_cn", "flags", "cn", "neighbors", "mutual")
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, bt):
    off = np.concatenate([[0], np.cumsum(bt.counts)]).astype(np.int32)
    return up(dev, bt.frac.reshape(-1, 3)), up(dev, bt.lattice), up(dev, off)


def launch(dev, bt):
    return co.result_to_numpy(co.coordination(*device_batch(dev, bt), bt.params))


def run(dev, name):
    """The kernel's arrays of one named batch (one launch each, cached)."""
    if name not in _RUN:
        _RUN[name] = launch(dev, cases.references()[name][0])
    return _RUN[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_the_case_list_is_what_the_tests_name():
    assert list(cases.references()) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_float32_restatement_bit_for_bit(dev, name):
    bt, r32, _ = cases.references()[name]
    got = run(dev, name)
    assert set(got) == set(co.RESULT_KEYS)
    for k in co.RESULT_KEYS:
        want = getattr(r32, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k, got[k].dtype, got[k].shape)
        assert np.array_equal(bits(got[k]), bits(want)), (name, k, np.flatnonzero((bits(got[k]) != bits(want)).reshape(len(want), -1).any(axis=1))[:8])


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_float64_restatement_on_the_guarded_crystals(dev, name):
    bt, _, r64 = cases.references()[name]
    got = run(dev, name)
    g, a = r64.guarded, np.repeat(r64.guarded, bt.counts)
    for k in ("n_bonds", "n_mutual", "min_cn", "max_cn", "flags"):
        assert np.array_equal(got[k][g], getattr(r64, k)[g]), (name, k)
    for k in ("cn", "neighbors", "mutual"):
        assert np.array_equal(got[k][a], getattr(r64, k)[a]), (name, k)
    bound = np.repeat(r64.bound, bt.counts)[a]
    for k in ("nearest", "farthest"):
        err = np.abs(got[k][a].astype(np.float64) - getattr(r64, k)[a])
        assert (err <= bound).all(), (name, k, float(err.max()))
    if bt.expect["cn"] is not None:
        assert got["cn"].tolist() == bt.expect["cn"], name
    if name != "known tol0":
        assert g.sum() >= {"flags": 3, "ragged": 63}.get(name, len(bt.counts))  # (the comparison is not vacuous)


def test_paths_and_flags_on_the_device(dev):
    bt, _, _ = cases.references()["flags"]
    got = run(dev, "flags")
    assert got["flags"][:7].tolist() == bt.expect["flags"][:7]
    first = np.concatenate([[0], np.cumsum(bt.counts)])
    assert got["nearest"][first[4]] == 20.0 and got["cn"][first[4]] == 0 and np.isnan(got["mean_cn"][1]) and got["min_cn"][1] == -1
    over = run(dev, "overflow")
    assert over["flags"].tolist() == [co.OVERFLOW] * 2 and over["cn"].tolist() == [12, 6]
    assert over["neighbors"][0].tolist() == [[0, -1, 0, 0], [0, -1, 0, 1], [0, -1, 1, 0], [0, 0, -1, 0]]
    large, lb = run(dev, "large"), cases.references()["large"][0]
    assert lb.counts[1] == co.cb.STAGED_ATOMS + 3 and (large["flags"] == 0).all() and (large["cn"] >= 1).all()
    skew = run(dev, "skewed")
    assert skew["neighbors"][0, :2].tolist() == [[0, -2, 1, 0], [0, 2, -1, 0]]
    # no crystals at all: nothing is launched
    empty = co.coordination(torch.empty((0, 3), device=dev), torch.empty((0, 3, 3), device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
    assert empty["flags"].shape == (0,) and empty["neighbors"].shape == (0, 24, 4)


def test_a_crystal_alone_gives_the_bits_it_gives_in_the_batch(dev):
    bt = cases.references()["ragged"][0]
    got = run(dev, "ragged")
    assert len(bt.counts) == 70 and bt.counts[cases.RAGGED_BIG] == 67
    first = np.concatenate([[0], np.cumsum(bt.counts)])
    for b in (cases.RAGGED_BIG, 0, 69):
        alone = launch(dev, cases.single(bt, b))
        for k in co.COORD_KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(got[k][b])), (b, k)
        for k in co.RESULT_KEYS[len(co.COORD_KEYS):]:
            assert np.array_equal(bits(alone[k]), bits(got[k][first[b]:first[b + 1]])), (b, k)
    again = launch(dev, bt)  # and a second launch of the whole batch
    for k in co.RESULT_KEYS:
        assert np.array_equal(bits(again[k]), bits(got[k])), k


@pytest.mark.parametrize("name", ["known", "ragged", "large"])
def test_smallest_nearest_against_the_screen(dev, name):
    """Per crystal, min_i nearest(i) against arreau_crystal_screen's min_distance at search_radius = cutoff: the same image range
    and the same contacts, but the screen forms a pair's difference from the smaller index only, so the two are not the same bits.
    Asserted: within screening.distance_bound (the derived bound of one float32 distance against the exact one; the two minima
    are each within it of the same exact minimum, and the coordination search also meets the screen's own expression, so its
    minimum is never the larger: the difference is one-sided).  Printed: both and the bound."""
    bt, _, r64 = cases.references()[name]
    got = run(dev, name)
    frac, lattice, off = device_batch(dev, bt)
    crit = sc.ScreenCriteria(min_distance=0.0, min_volume=0.0, search_radius=bt.params.cutoff, mask_type=-1, max_shells=bt.params.max_shells)
    screened = sc.metrics_to_numpy(sc.screen(frac, lattice, off, None, crit))
    first = np.concatenate([[0], np.cumsum(bt.counts)])
    for b, n in enumerate(bt.counts):
        assert (got["flags"][b] & (co.NONFINITE | co.CELL | co.EMPTY)) == 0 and (screened["flags"][b] & (sc.NONFINITE | sc.CELL)) == 0
        mine, theirs = float(got["nearest"][first[b]:first[b + 1]].min()), float(screened["min_distance"][b])
        print(name, b, mine, theirs, r64.bound[b])
        assert mine <= theirs and theirs - mine <= r64.bound[b], (name, b, mine, theirs)


def test_sample_with_coordination(dev, fused_model):
    m, _ = fused_model
    params = co.CoordinationParams(tol=0.15, cutoff=5.0, max_neighbors=16)
    out = []
    for kw in ({}, dict(coordination=True), dict(coordination=None), dict(coordination=params, find_symmetry=True, screen=True, reduce_cell=True),
               dict(find_symmetry=True, screen=True, reduce_cell=True)):
        torch.manual_seed(3)
        np.random.seed(3)
        r = m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)
        out.append((r, torch.random.get_rng_state(), np.random.uniform()))
    plain = out[0][0]
    for r, rng, after in out[1:]:
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and np.array_equal(plain.num_atoms, r.num_atoms)
        assert torch.equal(out[0][1], rng) and out[0][2] == after
    a, none, every, others = out[1][0], out[2][0], out[3][0], out[4][0]
    assert plain.coordination is None and none.coordination is None and others.coordination is None
    assert a.metrics is None and a.symmetry is None and a.reduced is None and a.conventional is None
    for field in ("metrics", "symmetry", "reduced"):  # every other instrument's arrays: as without the keyword
        x, y = getattr(every, field), getattr(others, field)
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))), (field, k)
    for r, p in ((a, None), (every, params)):  # the engine-free entry point on the returned crystals
        c = r.coordination
        assert set(c) == set(co.STORED_KEYS) and c["cn"].shape == (12,) and c["flags"].shape == (3,)
        assert c["neighbors"].shape == (12, 24 if p is None else 16, 4) and np.array_equal(c["species"], np.rint(r.atomic_numbers).astype(np.int64))
        direct = co.coordination_sample_result(r, p, dev)
        for k in co.STORED_KEYS:
            assert np.array_equal(bits(c[k]), bits(direct[k])), k
        ref = co.coordination_reference_f32(r.frac_x, r.lattice, r.num_atoms, p)
        for k in INTEGERS + ("nearest", "farthest", "mean_cn"):
            assert np.array_equal(bits(c[k]), bits(getattr(ref, k))), k


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_write_and_print_the_same_numbers(dev, tmp_path):
    """generate --coordination, then screen --coordination --out on the file it wrote: each a fresh process."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out, out2 = str(tmp_path / "out" / "crystals.npz"), str(tmp_path / "again.npz")
    flags = ["--coordination", "--cn_tol", "0.2", "--cn_cutoff", "5.5"]
    text = _child(["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "10",
                   "--seed", "5", "--out", out] + flags, 300)
    lines = [ln for ln in text.splitlines() if ln.startswith("coordination ")]
    assert len(lines) == 2 and re.match(r"coordination rank 0: 5 crystals, \d+ atoms; cn ", lines[0]) and lines[1].startswith("coordination total: 5 crystals"), text
    assert "screen rank" not in text and "conventional" not in text, text  # the other instruments print nothing unasked
    res = load_sample_results_from_hdf5(out)
    c = res.coordination
    assert set(c) == set(co.STORED_KEYS) and c["cn"].shape == (30,) and c["neighbors"].shape == (30, 24, 4) and res.metrics is None
    ref = co.coordination_reference_f32(res.frac_x, res.lattice, res.num_atoms, co.CoordinationParams(tol=0.2, cutoff=5.5))
    for k in INTEGERS + ("nearest", "farthest", "mean_cn"):
        assert np.array_equal(bits(c[k]), bits(getattr(ref, k))), k
    text2 = _child(["arreau_amd.screen", out, "--out", out2] + flags, 120)
    lines2 = [ln for ln in text2.splitlines() if ln.startswith("coordination ")]
    assert lines2 == lines, (lines, lines2)
    back = load_sample_results_from_hdf5(out2)
    for k in co.STORED_KEYS:
        assert np.array_equal(bits(back.coordination[k]), bits(c[k])), k
    assert back.metrics is not None  # (the screen always runs there)
    # a file of the known structures (a synthetic checkpoint's crystals are mostly a gas): the textbook numbers, printed and stored
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import save_sample_results_to_hdf5
    bt, r32, _ = cases.references()["known"]
    num = np.array(bt.counts, dtype=np.int64)
    known, out3 = str(tmp_path / "known.npz"), str(tmp_path / "known_out.npz")
    save_sample_results_to_hdf5(SampleResult(frac_x=bt.frac.astype(np.float64), atomic_numbers=bt.species.astype(np.float64),
                                             lattice=bt.lattice.astype(np.float64), num_atoms=num, idx_start=np.cumsum(num) - num), known)
    text3 = _child(["arreau_amd.screen", known, "--coordination", "--out", out3], 120)
    assert "coordination total: 10 crystals, 36 atoms; cn 2: 3, 4: 12, 6: 10, 8: 7, 12: 4; mean cn " in text3 and "Z 20: 8.00" in text3, text3
    stored = load_sample_results_from_hdf5(out3).coordination
    for k in INTEGERS + ("nearest", "farthest", "mean_cn"):
        assert np.array_equal(bits(stored[k]), bits(getattr(r32, k))), k
    assert np.array_equal(stored["species"], bt.species)


def test_argument_errors_touch_nothing(dev):
    bt = cases.single(cases.references()["known"][0], 5)
    frac, lattice, off = device_batch(dev, bt)
    with pytest.raises(ValueError, match="coordination: offsets"):
        co.coordination(frac, lattice, off.to(torch.int64))
    out = co.coordination(frac, lattice, off)
    before = {k: out[k].clone() for k in co.RESULT_KEYS}
    r = _hip.CoordinationResultC(*[_hip.ptr(out[k]).value for k in co.RESULT_KEYS])
    good = (0.1, 6.0, 24, 8)
    call = _hip.lib().arreau_crystal_coordination
    EINVAL = -1  # ARREAU_EINVAL
    B, N = 1, int(frac.shape[0])
    trials = [(B, N, None, ctypes.byref(r)), (B, N, good, None), (-1, N, good, ctypes.byref(r)), (B, -1, good, ctypes.byref(r)),
              (B, N, good, ctypes.byref(_hip.CoordinationResultC()))]
    trials += [(B, N, bad, ctypes.byref(r)) for bad in ((-0.1, 6.0, 24, 8), (float("nan"), 6.0, 24, 8), (0.1, 0.0, 24, 8), (0.1, float("inf"), 24, 8),
                                                       (0.1, 6.0, 0, 8), (0.1, 6.0, 65, 8), (0.1, 6.0, 24, 0), (0.1, 6.0, 24, 9))]
    for b, n, p, res in trials:
        c = ctypes.byref(_hip.CoordinationParamsC(*p)) if p is not None else None
        assert call(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), b, n, c, res, _hip.stream_ptr(dev)) == EINVAL, (b, n, p)
        assert b"arreau_crystal_coordination" in _hip.lib().arreau_last_error()
    c = ctypes.byref(_hip.CoordinationParamsC(*good))
    assert call(None, _hip.ptr(lattice), _hip.ptr(off), B, N, c, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    assert call(None, None, None, 0, 0, c, ctypes.byref(_hip.CoordinationResultC()), _hip.stream_ptr(dev)) == 0  # B == 0: OK
    torch.cuda.synchronize()
    for k in co.RESULT_KEYS:
        assert torch.equal(before[k], out[k]), k


def test_sample_takes_the_keyword_and_the_symbol_is_exported(fused_model):
    """What fails without the feature: sample(coordination=...) is a TypeError and the entry point is not in the library."""
    import inspect
    m, _ = fused_model
    assert "coordination" in inspect.signature(m.sample).parameters
    assert "arreau_crystal_coordination" in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_coordination")
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_coordination(" in fh.read()
