"""The powder patterns on the device (arreau_crystal_xrd, csrc/xrd.hip) on the batches of tests/xrd_cases.py: against the float64
restatement (n_reflections and flags equal -- no crystal sits within 1e-9 of a d* cut, test_xrd_cpu.py --, the pattern within
xrd.F32_BOUND of its maximum: 16 times the deviation measured on the CPU by tools/exp/xrd_f32_deviation.py, never from the
kernel's output), the invariance pairs against each other on the device's own numbers, a crystal alone against the same crystal
first, last and in the middle of the 70-crystal batch bit for bit, the three scattering modes, sample(xrd=...), the two command
lines, the argument errors and the export.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import xrd
from tests import xrd_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, bt):
    off = np.concatenate([[0], np.cumsum(bt.counts)]).astype(np.int32)
    return up(dev, bt.frac.reshape(-1, 3)), up(dev, bt.lattice), up(dev, off), up(dev, bt.species.astype(np.int32))


def launch(dev, bt):
    return xrd.result_to_numpy(xrd.xrd(*device_batch(dev, bt), bt.params))


def run(dev, name):
    """The kernel's arrays of one named batch (one launch each, cached)."""
    if name not in _RUN:
        _RUN[name] = launch(dev, cases.batch(name))
    return _RUN[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("name", cases.BATCHES)
def test_kernel_matches_the_float64_restatement(dev, name):
    bt, r = cases.reference(name)
    got = run(dev, name)
    assert set(got) == set(xrd.RESULT_KEYS) and got["pattern"].shape == (len(bt.counts), bt.params.n_points)
    assert got["pattern"].dtype == np.float32 and got["n_reflections"].dtype == np.int32 and got["flags"].dtype == np.int32
    ok = r.flags == 0
    assert (r.margin[ok] >= xrd.MARGIN_GUARD).all()  # no crystal is left out of the exact comparison
    assert np.array_equal(got["flags"], r.flags) and np.array_equal(got["n_reflections"], r.n_reflections), name
    assert np.isnan(got["pattern"][~ok]).all() and np.isnan(got["volume"][~ok]).all() and np.isnan(got["weight_sum"][~ok]).all()
    assert np.array_equal(bits(got["volume"][ok]), bits(r.volume[ok])) and np.array_equal(bits(got["weight_sum"][ok]), bits(r.weight_sum[ok]))
    top = cases.scale(r)
    err = np.abs(got["pattern"][ok].astype(np.float64) - r.pattern[ok]).max(axis=1, initial=0.0) / top[ok]
    print(name, "largest |P_dev - P_64| / max(P_64):", float(err.max(initial=0.0)), "bound", xrd.F32_BOUND)
    assert not np.isnan(got["pattern"][ok]).any() and (err <= xrd.F32_BOUND).all(), (name, err.max(), int(np.argmax(err)))


def test_the_descriptions_of_one_crystal_agree_on_the_device(dev):
    """The three pairs against each other: to twice the bound at the default parameters.  On the other grids and widths they are
    allowed, on top of it, what the float64 restatement's own two patterns differ by: float32 holds the second description's
    cell and coordinates to 2^-24 only, so the two inputs are not the same crystal, and a reflection moved by 5e-6 degrees changes
    the flank of a peak of sigma 0.025 degrees by 2.9e-5 of the maximum (`narrow`, in float64 too; 2.7e-6 at the default width)."""
    for name in ("invariance", "points 2", "points 257", "points 4096", "narrow", "wide", "b_iso"):
        got, r = run(dev, name), cases.reference(name)[1]
        for a, b in cases.INVARIANCE_PAIRS:
            i, j = cases.INVARIANCE_NAMES.index(a), cases.INVARIANCE_NAMES.index(b)
            diff = np.abs(got["pattern"][i].astype(np.float64) - got["pattern"][j]).max()
            own = 0.0 if name == "invariance" else np.abs(r.pattern[i] - r.pattern[j]).max()
            assert diff <= 2.0 * xrd.F32_BOUND * cases.scale(r)[i] + own, (name, a, b, diff / cases.scale(r)[i], own / cases.scale(r)[i])
    got = run(dev, "invariance")
    assert got["n_reflections"].tolist()[:2] == [170, 50] and got["n_reflections"][2] == got["n_reflections"][3] < got["n_reflections"][4]
    peak = xrd.sample_arrays(got)["two_theta_peak"]
    assert abs(peak[0] - 43.4) < 0.026 and abs(peak[0] - peak[1]) < 0.051 and max(abs(peak[2] - peak[3]), abs(peak[2] - peak[4])) < 0.051  # (a grid step)


def test_flags_and_textbook_absences_on_the_device(dev):
    got = run(dev, "flags")
    assert got["flags"].tolist() == cases.FLAGS_EXPECTED and (got["n_reflections"][:4] == 0).all() and got["n_reflections"][4] > 0
    assert np.isnan(got["pattern"][:4]).all() and got["volume"][4] == 27.0 and got["weight_sum"][4] == 13.0
    # an amplitude that is not finite; an index cap of 1
    one = cases.single(cases.batch("flags"), 4)
    frac, lattice, off, _ = device_batch(dev, one)
    bad = xrd.result_to_numpy(xrd.xrd(frac, lattice, off, torch.full((1,), float("inf"), device=dev), xrd.XrdParams(scattering="weights")))
    assert bad["flags"].tolist() == [xrd.NONFINITE] and np.isnan(bad["pattern"]).all()
    assert launch(dev, cases._batch("cap", cases.flag_crystals()[4:], xrd.XrdParams(max_index=1)))["flags"].tolist() == [xrd.RANGE]
    # bcc: nothing at (100); fcc: nothing at (100) and (110); both relative to the float32 bound, not to 1e-12
    text, g = run(dev, "textbook"), xrd.grid()
    near = lambda b, a, hkl: float(text["pattern"][b][int(np.argmin(np.abs(g - 2.0 * np.degrees(np.arcsin(0.5 * 1.54184 * np.sqrt(np.sum(np.square(hkl))) / a)))))])
    bcc, fcc = cases.TEXTBOOK_NAMES.index("bcc"), cases.TEXTBOOK_NAMES.index("fcc")
    assert near(bcc, cases.A_FE, (1, 0, 0)) <= xrd.F32_BOUND * text["pattern"][bcc].max() < near(bcc, cases.A_FE, (1, 1, 0))
    assert max(near(fcc, cases.A_CU, (1, 0, 0)), near(fcc, cases.A_CU, (1, 1, 0))) <= xrd.F32_BOUND * text["pattern"][fcc].max()
    # no crystals at all: nothing is launched
    empty = xrd.xrd(torch.empty((0, 3), device=dev), torch.empty((0, 3, 3), device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                    torch.empty(0, device=dev))
    assert empty["pattern"].shape == (0, 1701) and empty["flags"].shape == (0,)


def test_a_crystal_alone_gives_the_bits_it_gives_in_the_batch(dev):
    bt = cases.batch("ragged")
    got = run(dev, "ragged")
    assert len(bt.counts) == 70
    for b in (0, cases.RAGGED_MIDDLE, 69):
        alone = launch(dev, cases.single(bt, b))
        for k in xrd.RESULT_KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(got[k][b])), (b, k)
    again = launch(dev, bt)  # and a second launch of the whole batch
    for k in xrd.RESULT_KEYS:
        assert np.array_equal(bits(again[k]), bits(got[k])), k
    big = cases.batch("large")  # past the staging: alone and behind another crystal
    pair = cases._batch("pair", [cases.random_crystal(3), cases.random_crystal(500, xrd.cb.STAGED_ATOMS + 1)])
    assert np.array_equal(big.frac, pair.frac[pair.counts[0]:])
    two = launch(dev, pair)
    for k in xrd.RESULT_KEYS:
        assert np.array_equal(bits(two[k][1]), bits(run(dev, "large")[k][0])), k


def test_the_three_scattering_modes(dev):
    bt = cases.batch("textbook")
    frac, lattice, off, z = device_batch(dev, bt)
    by_z = run(dev, "textbook")
    as_weights = xrd.result_to_numpy(xrd.xrd(frac, lattice, off, z.to(torch.float32), xrd.XrdParams(scattering="weights")))
    from_float = xrd.result_to_numpy(xrd.xrd(frac, lattice, off, z.to(torch.float64)))
    for k in xrd.RESULT_KEYS:
        assert np.array_equal(bits(as_weights[k]), bits(by_z[k])) and np.array_equal(bits(from_float[k]), bits(by_z[k])), k
    unit = xrd.result_to_numpy(xrd.xrd(frac, lattice, off, None, xrd.XrdParams(scattering="unit")))
    ones = xrd.result_to_numpy(xrd.xrd(frac, lattice, off, torch.ones_like(z, dtype=torch.float32), xrd.XrdParams(scattering="weights")))
    for k in xrd.RESULT_KEYS:
        assert np.array_equal(bits(unit[k]), bits(ones[k])), k
    assert unit["weight_sum"].tolist() == [float(n) for n in bt.counts] and by_z["weight_sum"][0] == 84.0
    with pytest.raises(ValueError, match="float32"):
        xrd.xrd(frac, lattice, off, z, xrd.XrdParams(scattering="weights"))
    with pytest.raises(ValueError, match="needs a"):
        xrd.xrd(frac, lattice, off, None)


def test_sample_with_xrd(dev, fused_model):
    m, _ = fused_model
    params = xrd.XrdParams(wavelength=0.7093, two_theta_min=3.0, two_theta_max=40.0, n_points=371, fwhm=0.15, scattering="unit")
    out = []
    for kw in ({}, dict(xrd=True), dict(xrd=None), dict(xrd=params, coordination=True, screen=True, reduce_cell=True),
               dict(coordination=True, screen=True, reduce_cell=True)):
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
    assert plain.xrd is None and none.xrd is None and others.xrd is None
    assert a.metrics is None and a.coordination is None and a.reduced is None and a.voronoi is None
    for field in ("metrics", "reduced", "coordination"):  # every other instrument's arrays: as without the keyword
        x, y = getattr(every, field), getattr(others, field)
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))), (field, k)
    for r, p in ((a, None), (every, params)):  # the engine-free entry point on the returned crystals
        c = r.xrd
        assert set(c) == set(xrd.STORED_KEYS) and c["pattern"].shape == (3, 1701 if p is None else 371) and c["flags"].shape == (3,)
        assert c["grid"].shape == (3, 5) and np.array_equal(c["grid"][0], xrd.grid_row(p or xrd.XrdParams()))  # the parameters reached the launch
        direct = xrd.xrd_sample_result(r, p, dev)
        for k in xrd.STORED_KEYS:
            assert np.array_equal(bits(c[k]), bits(direct[k])), k
        q = p or xrd.XrdParams()
        ref = xrd.xrd_reference(r.frac_x, r.lattice, r.num_atoms, xrd.host_weights(r.atomic_numbers, q), q)
        ok = (ref.flags == 0) & (ref.margin >= xrd.MARGIN_GUARD)
        assert np.array_equal(c["flags"], ref.flags) and np.array_equal(c["n_reflections"][ok], ref.n_reflections[ok])
        err = np.abs(c["pattern"][ok].astype(np.float64) - ref.pattern[ok]).max(axis=1, initial=0.0)
        assert (err <= xrd.F32_BOUND * cases.scale(ref)[ok]).all()
        if p is not None:
            assert c["weight_sum"][ok].tolist() == [float(n) for n in np.asarray(r.num_atoms)[ok]]


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_write_and_print_the_same_numbers(dev, tmp_path):
    """generate --xrd, then screen --xrd --xrd_against --out on a file of the textbook cells: each a fresh process."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out = str(tmp_path / "out" / "crystals.npz")
    flags = ["--xrd", "--xrd_fwhm", "0.3", "--xrd_points", "851", "--xrd_two_theta_max", "80"]
    text = _child(["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "10",
                   "--seed", "5", "--out", out] + flags, 300)
    lines = [ln for ln in text.splitlines() if ln.startswith("xrd ")]
    assert len(lines) == 2 and re.match(r"xrd rank 0: 5 crystals, \d patterns; mean n_reflections ", lines[0]) and lines[1].startswith("xrd total: 5 crystals"), text
    assert "voronoi rank" not in text and "coordination rank" not in text, text  # the other instruments print nothing unasked
    res = load_sample_results_from_hdf5(out)
    c = res.xrd
    p = xrd.XrdParams(fwhm=0.3, n_points=851, two_theta_max=80.0)
    assert set(c) == set(xrd.STORED_KEYS) and c["pattern"].shape == (5, 851) and np.array_equal(c["grid"][4], xrd.grid_row(p)) and res.voronoi is None
    ref = xrd.xrd_reference(res.frac_x, res.lattice, res.num_atoms, xrd.host_weights(res.atomic_numbers, p), p)
    ok = (ref.flags == 0) & (ref.margin >= xrd.MARGIN_GUARD)
    assert np.array_equal(c["flags"], ref.flags) and np.array_equal(c["n_reflections"][ok], ref.n_reflections[ok])
    assert (np.abs(c["pattern"][ok].astype(np.float64) - ref.pattern[ok]).max(axis=1, initial=0.0) <= xrd.F32_BOUND * cases.scale(ref)[ok]).all()
    # a file of the textbook cells against itself: six patterns, printed and stored, every pair at distance 0
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import save_sample_results_to_hdf5
    bt, r = cases.reference("textbook")
    num = np.array(bt.counts, dtype=np.int64)
    known, out3 = str(tmp_path / "known.npz"), str(tmp_path / "known_out.npz")
    save_sample_results_to_hdf5(SampleResult(frac_x=bt.frac.astype(np.float64), atomic_numbers=bt.species.astype(np.float64),
                                             lattice=bt.lattice.astype(np.float64), num_atoms=num, idx_start=np.cumsum(num) - num), known)
    text3 = _child(["arreau_amd.screen", known, "--xrd", "--xrd_against", known, "--out", out3], 120)
    assert "xrd total: 6 crystals, 6 patterns; mean n_reflections " in text3 and "flags none" in text3, text3
    assert "xrd against: 6 / 6 pairs; paired distance mean 0.000000, median 0.000000" in text3, text3
    stored = load_sample_results_from_hdf5(out3).xrd
    assert np.array_equal(stored["n_reflections"], r.n_reflections) and (stored["flags"] == 0).all()
    assert (np.abs(stored["pattern"].astype(np.float64) - r.pattern).max(axis=1) <= xrd.F32_BOUND * cases.scale(r)).all()


def test_argument_errors_touch_nothing(dev):
    bt = cases.single(cases.batch("textbook"), 1)
    frac, lattice, off, z = device_batch(dev, bt)
    with pytest.raises(ValueError, match="xrd: offsets"):
        xrd.xrd(frac, lattice, off.to(torch.int64), z)
    w = z.to(torch.float32)
    out = xrd.xrd(frac, lattice, off, w, xrd.XrdParams(scattering="weights"))
    before = {k: out[k].clone() for k in xrd.RESULT_KEYS}
    r = _hip.XrdResultC(*[_hip.ptr(out[k]).value for k in xrd.RESULT_KEYS])
    good = (1.54184, 5.0, 90.0, 0.2, 0.0, 1701, 64)
    change = lambda i, v: good[:i] + (v,) + good[i + 1:]
    call = _hip.lib().arreau_crystal_xrd
    EINVAL = -1  # ARREAU_EINVAL
    B, N = 1, int(frac.shape[0])
    trials = [(B, N, None, ctypes.byref(r)), (B, N, good, None), (-1, N, good, ctypes.byref(r)), (B, -1, good, ctypes.byref(r)),
              (B, N, good, ctypes.byref(_hip.XrdResultC()))]
    trials += [(B, N, bad, ctypes.byref(r)) for bad in (
        change(0, 0.0), change(0, -1.0), change(0, float("nan")), change(0, float("inf")), change(1, -0.5), change(1, 90.0), change(1, float("nan")),
        change(2, 160.5), change(2, float("nan")), change(3, 0.0), change(3, -0.2), change(3, float("nan")), change(3, 3.93), change(4, -0.1),
        change(4, float("nan")), change(4, float("inf")), change(5, 1), change(5, 4097), change(6, 0), change(6, 128))]
    args = lambda: (_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), _hip.ptr(w))
    for b, n, p, res in trials:
        c = ctypes.byref(_hip.XrdParamsC(*p)) if p is not None else None
        assert call(*args(), b, n, c, res, _hip.stream_ptr(dev)) == EINVAL, (b, n, p)
        assert b"arreau_crystal_xrd" in _hip.lib().arreau_last_error()
    c = ctypes.byref(_hip.XrdParamsC(*good))
    assert call(None, _hip.ptr(lattice), _hip.ptr(off), _hip.ptr(w), B, N, c, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    assert call(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), None, B, N, c, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    one_null = _hip.XrdResultC(*[_hip.ptr(out[k]).value if k != "weight_sum" else None for k in xrd.RESULT_KEYS])
    assert call(*args(), B, N, c, ctypes.byref(one_null), _hip.stream_ptr(dev)) == EINVAL
    assert call(None, None, None, None, 0, 0, c, ctypes.byref(_hip.XrdResultC()), _hip.stream_ptr(dev)) == 0  # B == 0: OK
    torch.cuda.synchronize()
    for k in xrd.RESULT_KEYS:
        assert torch.equal(before[k], out[k]), k


def test_sample_takes_the_keyword_and_the_symbol_is_exported(fused_model):
    """What fails without the feature: sample(xrd=...) is a TypeError and the entry point is not in the library."""
    import inspect
    m, _ = fused_model
    assert "xrd" in inspect.signature(m.sample).parameters
    assert "arreau_crystal_xrd" in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_xrd")
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_xrd(" in fh.read()
