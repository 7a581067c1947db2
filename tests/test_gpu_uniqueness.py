"""Duplicate detection on the device (arreau_crystal_fingerprint, arreau_fingerprint_match): the fingerprint within the bound of
the float64 restatement on one ragged batch (1 to 257 atoms, 1 to 9 species, every flag), bitwise repeatability and independence
of the place in the batch, the seven equivalent variants matched to the first, the match against match_reference at sizes that are
no multiple of the tile, argument errors, sample(unique=...) and the two command lines.  The bound is uniqueness.FHAT_BOUND /
D_BOUND: four times the float32 restatement's measured deviation (test_uniqueness_cpu.py).  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import screening as sc
from arreau_amd.diffusion import uniqueness as uq
from tests import uniqueness_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_KEYS = ("fingerprint", "species", "counts", "flags")
MATCH_INTS, MATCH_REALS = ("duplicate_of", "nearest"), ("distance", "nearest_distance")


def run_fingerprint(dev, b, params=None):
    off = np.concatenate([[0], np.cumsum(b.counts)]).astype(np.int32)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return uq.fingerprint(up(b.frac), up(b.lattice), up(off), up(b.types), params if params is not None else cases.params())


def host(s):
    return {k: v.cpu().numpy() for k, v in s.items()}


def rows(s, B):
    return {k: s[k][:B].contiguous() for k in SET_KEYS}


@pytest.fixture(scope="module")
def match_fingerprints(dev):
    x, y = cases.match_sets()
    return run_fingerprint(dev, x), run_fingerprint(dev, y)


def test_fingerprint_within_the_bound_of_the_f64_restatement(dev):
    b, ref = cases.ragged_batch(), cases.reference_f64("ragged")
    got = host(run_fingerprint(dev, b))
    assert got["flags"].tolist() == ref.flags.tolist() == cases.RAGGED_FLAGS
    assert got["species"].tolist() == ref.species.tolist() and got["counts"].tolist() == ref.counts.tolist()
    assert got["fingerprint"].dtype == np.float32 and got["fingerprint"].shape == (len(b.counts), uq.ROW)
    dev_rows = np.abs(got["fingerprint"].astype(np.float64) - ref.fingerprint).max(axis=1)
    for k, name in enumerate(cases.RAGGED_NAMES):
        print(f"{name}: n {b.counts[k]} contacts {ref.n_contacts[k]} flags {got['flags'][k]} max |f - f64| {dev_rows[k]:.3e} (bound {uq.FHAT_BOUND:.3e})")
    assert (dev_rows <= uq.FHAT_BOUND).all(), dev_rows
    for k, f in enumerate(cases.RAGGED_FLAGS):
        assert not got["fingerprint"][k].any() if f else abs(np.linalg.norm(got["fingerprint"][k].astype(np.float64)) - 1) < 1e-5
    # fewer bins and another smearing: the same comparison on the small members
    p = uq.FingerprintParams(r_max=5.0, n_bins=40, sigma=0.15)
    small = cases.batch("small", b.crystals[:4] + b.crystals[7:8])
    r = uq.fingerprint_reference_f64(small.frac, small.lattice, small.counts, small.types, p, details=True)
    g = host(run_fingerprint(dev, small, p))
    assert (r.near_cut == 0).all() and g["flags"].tolist() == r.flags.tolist()
    assert np.abs(g["fingerprint"].astype(np.float64) - r.fingerprint).max() <= uq.FHAT_BOUND
    assert not g["fingerprint"].reshape(-1, uq.COMPONENTS, uq.BINS)[:, :, 40:].any()


def test_rows_are_repeatable_and_independent_of_the_place_in_the_batch(dev):
    b = cases.ragged_batch()
    one, two = host(run_fingerprint(dev, b)), host(run_fingerprint(dev, b))
    for k in SET_KEYS:
        assert one[k].tobytes() == two[k].tobytes(), k
    assert one["fingerprint"][3].tobytes() == one["fingerprint"][12].tobytes()  # the same crystal twice in the batch
    for k in (3, 5):  # 20 atoms; 257 atoms (positions read through global memory)
        c, others = b.crystals[k], [b.crystals[q] for q in (2, 4, 0, 7)]
        alone = host(run_fingerprint(dev, cases.batch("alone", [c])))
        first = host(run_fingerprint(dev, cases.batch("first", [c] + others)))
        last = host(run_fingerprint(dev, cases.batch("last", others + [c])))
        assert alone["fingerprint"][0].any()
        assert alone["fingerprint"][0].tobytes() == first["fingerprint"][0].tobytes() == last["fingerprint"][-1].tobytes() == one["fingerprint"][k].tobytes()
        assert alone["counts"][0].tolist() == last["counts"][-1].tolist()


def test_the_equivalent_variants_match_the_first(dev):
    b, ref = cases.invariance_set(), cases.reference_f64("invariance")
    fp = run_fingerprint(dev, b)
    got, want = host(uq.match(fp)), uq.match_reference(ref)
    names = cases.INVARIANCE_NAMES
    print("d to the base:", {n: float(got["nearest_distance"][k]) for k, n in enumerate(names)})
    assert got["duplicate_of"].tolist() == want.duplicate_of.tolist() == [-1] + [0] * 6 + [-1] * 4
    assert got["unique"].tolist() == want.unique.tolist() and not got["flags"].any()
    assert np.abs(got["distance"][1:7]).max() <= uq.D_BOUND
    cscl = names.index("cscl")
    assert got["nearest"][cscl] >= 0 and abs(float(got["nearest_distance"][cscl]) - want.nearest_distance[cscl]) <= uq.D_BOUND
    assert got["nearest_distance"][cscl] > 10 * uq.DEFAULT_TOLERANCE
    for n in ("ab2", "a2b", "other_pair"):
        k = names.index(n)
        assert got["nearest"][k] == -1 and np.isinf(got["nearest_distance"][k]) and np.isinf(got["distance"][k])
    assert np.abs(host(fp)["fingerprint"].astype(np.float64) - ref.fingerprint).max() <= uq.FHAT_BOUND


def _assert_match(got, want, what):
    for k in MATCH_INTS:
        assert got[k].dtype == np.int32 and got[k].tolist() == getattr(want, k).tolist(), (what, k)
    for k in MATCH_REALS:
        g, w = got[k].astype(np.float64), getattr(want, k)
        assert (np.isinf(g) == np.isinf(w)).all(), (what, k)
        fin = np.isfinite(w)
        worst = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
        print(f"{what}: {k} worst {worst:.3e} (bound {uq.D_BOUND:.3e})")
        assert worst <= uq.D_BOUND, (what, k)
    assert got["unique"].tolist() == want.unique.tolist() and got["flags"].tolist() == want.flags.tolist(), what


@pytest.mark.parametrize("Bx", cases.MATCH_SIZES)
def test_self_match_against_the_reference(dev, match_fingerprints, Bx):
    got = host(uq.match(rows(match_fingerprints[0], Bx)))
    _assert_match(got, uq.match_reference(cases.prefix(cases.reference_f64("match_x"), Bx)), f"self {Bx}")
    if Bx == 70:
        assert got["duplicate_of"][[12, 20, 25, 35, 50, 69]].tolist() == [3, 3, 5, 17, 3, 0] and got["duplicate_of"][[9, 40, 30]].tolist() == [-1] * 3
        assert (got["duplicate_of"] >= 0).sum() >= 7 and (got["nearest"] >= 0).sum() > 50


@pytest.mark.parametrize("By", cases.MATCH_SIZES)
@pytest.mark.parametrize("Bx", cases.MATCH_SIZES)
def test_two_set_match_against_the_reference(dev, match_fingerprints, Bx, By):
    x, y = match_fingerprints
    got = host(uq.match(rows(x, Bx), rows(y, By)))
    want = uq.match_reference(cases.prefix(cases.reference_f64("match_x"), Bx), cases.prefix(cases.reference_f64("match_y"), By))
    _assert_match(got, want, f"{Bx} x {By}")
    if Bx == By == 70:
        assert got["duplicate_of"][[0, 7, 31, 3, 12, 61]].tolist() == [2, 16, 33, 65, 65, 48]
        other = host(uq.match(rows(y, 70), rows(x, 70)))  # the other way round
        _assert_match(other, uq.match_reference(cases.reference_f64("match_y"), cases.reference_f64("match_x")), "y x")


def test_argument_errors_touch_nothing(dev):
    L = _hip.lib()
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    frac, lat, off = torch.rand(3, 3, **f32), torch.eye(3, **f32)[None] * 5, torch.tensor([0, 3], **i32)
    types = torch.zeros(3, **i32)
    out = {"fingerprint": torch.full((1, uq.ROW), 7.0, **f32), "species": torch.full((1, 8), 7, **i32), "counts": torch.full((1, 8), 7, **i32),
           "flags": torch.full((1,), 7, **i32)}
    res = _hip.FingerprintResultC(*[_hip.ptr(out[k]).value for k in SET_KEYS])

    def fp(params=(6.0, 0.1, 64, 8), frac=frac, types=types, lat=lat, off=off, B=1, N=3, res=res, null_params=False):
        c = _hip.FingerprintParamsC(*params)
        return L.arreau_crystal_fingerprint(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lat), _hip.ptr(off), B, N, None if null_params else ctypes.byref(c),
                                            ctypes.byref(res) if res is not None else None, _hip.stream_ptr(dev))
    for kw, word in [(dict(params=(6.0, 0.1, 0, 8)), "n_bins"), (dict(params=(6.0, 0.1, 65, 8)), "n_bins"), (dict(params=(0.0, 0.1, 64, 8)), "r_max"),
                     (dict(params=(float("nan"), 0.1, 64, 8)), "r_max"), (dict(params=(6.0, -0.1, 64, 8)), "sigma"),
                     (dict(params=(6.0, float("inf"), 64, 8)), "sigma"), (dict(params=(6.0, 0.1, 64, 9)), "max_shells"),
                     (dict(null_params=True), "null"), (dict(res=None), "null"), (dict(B=-1), "size"), (dict(lat=None), "null pointer"),
                     (dict(types=None), "null pointer"), (dict(off=None), "null pointer"),
                     (dict(res=_hip.FingerprintResultC(*[_hip.ptr(out[k]).value if k != "counts" else None for k in SET_KEYS])), "result array")]:
        assert fp(**kw) == -1, kw
        assert word in L.arreau_last_error().decode(), (kw, L.arreau_last_error().decode())
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())  # nothing was launched
    assert fp(B=0, N=0, lat=None, off=None, frac=None, types=None) == 0
    assert fp() == 0
    torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0 and out["species"][0].tolist() == [0] + [-1] * 7 and out["counts"][0].tolist() == [1] + [0] * 7

    m = {"duplicate_of": torch.full((1,), 7, **i32), "distance": torch.full((1,), 7.0, **f32), "nearest": torch.full((1,), 7, **i32),
         "nearest_distance": torch.full((1,), 7.0, **f32)}
    keys = ("duplicate_of", "distance", "nearest", "nearest_distance")
    mres = _hip.MatchResultC(*[_hip.ptr(m[k]).value for k in keys])

    def match(x=res, Bx=1, y=None, By=0, tol=0.01, mres=mres):
        return L.arreau_fingerprint_match(ctypes.byref(x) if x is not None else None, Bx, ctypes.byref(y) if y is not None else None, By, tol,
                                          ctypes.byref(mres) if mres is not None else None, _hip.stream_ptr(dev))
    for kw, word in [(dict(tol=-0.1), "tolerance"), (dict(tol=1.5), "tolerance"), (dict(tol=float("nan")), "tolerance"), (dict(x=None), "null"),
                     (dict(mres=None), "null"), (dict(Bx=-1), "size"), (dict(y=res, By=-1), "size"),
                     (dict(x=_hip.FingerprintResultC(None, *[_hip.ptr(out[k]).value for k in SET_KEYS[1:]])), "set array"),
                     (dict(mres=_hip.MatchResultC(*[_hip.ptr(m[k]).value if k != "nearest" else None for k in keys])), "result array")]:
        assert match(**kw) == -1, kw
        assert word in L.arreau_last_error().decode(), (kw, L.arreau_last_error().decode())
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in m.values())
    assert match(Bx=0) == 0 and match() == 0 and match(y=res, By=0) == 0
    torch.cuda.synchronize()
    assert int(m["duplicate_of"][0]) == -1 and int(m["nearest"][0]) == -1 and bool(torch.isinf(m["distance"][0]))
    with pytest.raises(ValueError, match="types"):
        uq.fingerprint(frac, lat, off, types.long())
    with pytest.raises(ValueError, match="tolerance"):
        uq.match(out, tolerance=2.0)


# ------------------------------------------------------------------------------------------------------------ the sampler
def _unique_again(dev, m, res, params):
    """The stand-alone calls on a returned state: its float32 arrays uploaded again, species as class indices."""
    zs = [int(z) for z in m.z_table_zs.tolist()]
    types = np.array([zs.index(int(z)) for z in res.atomic_numbers], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(res.num_atoms)]).astype(np.int32)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return uq.uniqueness_to_numpy(uq.unique_batch(up(res.frac_x.astype(np.float32)), up(res.lattice.astype(np.float32)), up(off), up(types), params))


def _sample(m, **kw):
    torch.manual_seed(11)
    np.random.seed(11)
    return m.sample([5, 9, 1, 14], 4, seed=99, num_steps=8, **kw)


def test_sample_with_uniqueness(dev, fused_model):
    """uniqueness equals the stand-alone calls on the returned state; unique=None returns what it returned, with uniqueness None;
    screen=True keeps exactly its metric keys."""
    m, _ = fused_model
    plain, uniq, both = _sample(m), _sample(m, unique=True), _sample(m, unique=uq.FingerprintParams(r_max=5.0, tolerance=0.02), screen=True)
    assert plain.uniqueness is None and plain.metrics is None and uniq.metrics is None
    for other in (uniq, both):
        for k in ("frac_x", "atomic_numbers", "lattice", "num_atoms"):
            a, b = np.asarray(getattr(plain, k)), np.asarray(getattr(other, k))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert set(both.metrics) == set(sc.METRIC_KEYS) | {"valid"}
    for res, p in ((uniq, uq.FingerprintParams()), (both, uq.FingerprintParams(r_max=5.0, tolerance=0.02))):
        again = _unique_again(dev, m, res, p)
        assert set(res.uniqueness) == set(again) == set(uq.UNIQUE_KEYS)
        for k, v in again.items():
            g = np.asarray(res.uniqueness[k])
            assert g.dtype == v.dtype and g.shape == v.shape == (4,) and g.tobytes() == v.tobytes(), k
        assert res.uniqueness["unique"].tolist() == ((res.uniqueness["duplicate_of"] < 0) & (res.uniqueness["flags"] == 0)).tolist()
    with pytest.raises(ValueError, match="unique must be"):
        _sample(m, unique="yes")


def test_sample_reports_crystals_that_are_identical_by_construction(dev, fused_model):
    """Three one-atom crystals of one constant species in one known cell: a lone atom's fingerprint depends on the cell alone
    (translation invariance), so the second and third duplicate the first."""
    from arreau_amd.diffusion.conditioning import SampleCondition
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.tools.atomic_number_table import SYMBOL_TO_Z
    m, _ = fused_model
    z = int(m.z_table_zs[1])
    symbol = {v: name for name, v in SYMBOL_TO_Z.items()}[z]
    cell = np.array([[4.0, 0, 0], [0.5, 4.5, 0], [0, 0.25, 5.0]])
    n = np.ones(3, np.int64)
    tmpl = SampleResult(num_atoms=n, frac_x=np.full((3, 3), 0.5), atomic_numbers=np.full(3, float(z)), lattice=np.stack([cell] * 3),
                        idx_start=np.arange(3))
    cond = SampleCondition.from_sample_result(tmpl, fix_lattice=True)
    torch.manual_seed(5)
    np.random.seed(5)
    res = m.sample(1, 3, condition=cond, seed=17, num_steps=8, use_constant_atomic_symbols=[symbol], unique=True)
    u = res.uniqueness
    assert u["flags"].tolist() == [0, 0, 0], u
    assert u["duplicate_of"].tolist() == [-1, 0, 0] and u["unique"].tolist() == [True, False, False]
    assert not np.array_equal(res.frac_x[0], res.frac_x[1])  # (the atoms ended elsewhere: the crystals are equal, not the arrays)


# ------------------------------------------------------------------------------------------------------------ the drivers
def _run(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=330)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def _line(stdout, word, who):
    m = re.search(rf"^{word} {who}: {word} (\d+) / attempted (\d+); (?:duplicates|matched) (\d+), flagged (\d+)", stdout, re.M)
    assert m, stdout
    return [int(v) for v in m.groups()]


def test_generate_unique_and_the_screen_command(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    common = ["--model_path", ckpt, "--num_atoms", "3", "--batch", "8", "--num_steps", "10", "--seed", "5", "--num_crystals", "12"]
    out = str(tmp_path / "u" / "crystals.npz")
    stdout = _run(["arreau_amd.generate"] + common + ["--unique", "--fp_tolerance", "0.02", "--out", out])
    res = load_sample_results_from_hdf5(out)
    total = _line(stdout, "unique", "total")
    assert _line(stdout, "unique", "rank 0") == total and total[1] == 12 and "screen total" not in stdout
    u = res.uniqueness
    assert res.metrics is None and u is not None and all(np.asarray(u[k]).shape == (12,) for k in uq.UNIQUE_KEYS)
    assert total == [int(u["unique"].sum()), 12, int((u["duplicate_of"] >= 0).sum()), int((u["flags"] != 0).sum())]
    # the stored arrays are the whole set's: the stand-alone call on the file gives them again
    again = uq.unique_sample_result(res, uq.FingerprintParams(tolerance=0.02), device=dev)
    assert all(np.asarray(u[k]).tobytes() == again[k].tobytes() for k in uq.UNIQUE_KEYS)
    # without --unique: today's keys, no line
    plain = str(tmp_path / "p" / "crystals.npz")
    stdout = _run(["arreau_amd.generate"] + common[:-2] + ["--num_crystals", "4", "--out", plain])
    with np.load(plain) as z:
        assert sorted(z.files) == ["atomic_numbers", "frac_x", "idx_start", "lattice", "num_atoms"] and "unique total" not in stdout
    # the screen command: uniqueness of the file, novelty against itself (every unflagged crystal finds itself) and against the other file
    rescreened = str(tmp_path / "r.npz")
    stdout = _run(["arreau_amd.screen", out, "--unique", "--fp_tolerance", "0.02", "--against", out, "--out", rescreened])
    assert _line(stdout, "unique", "total") == total and "screen total:" in stdout
    novel = _line(stdout, "novel", "total")
    assert novel[0] == 0 and novel[1] == 12 and novel[2] == 12 - total[3] and "against 12 crystals" in stdout
    back = load_sample_results_from_hdf5(rescreened)
    assert back.metrics is not None and all(np.asarray(back.uniqueness[k]).tobytes() == np.asarray(u[k]).tobytes() for k in uq.UNIQUE_KEYS)
