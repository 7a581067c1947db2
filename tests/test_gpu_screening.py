"""The structural screen on the device (arreau_crystal_screen): bit for bit against the float32 restatement on all six outputs --
the CPU test's random set and hand-made cases, a crystal above the LDS staging limit, a batch of 1,024 crystals --, within the
derived bound against the float64 restatement, argument errors, sample(screen=...) in every noise mode and with a schedule, a
lattice system and a symmetry spec, and generate.py --require_valid.  Needs an MI355X: `-m gpu`."""
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
from tests import screening_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS, INTS = ("min_distance", "volume", "number_density"), ("pair", "n_close", "flags")


def run_kernel(dev, batch, crit, with_types=True):
    off = np.concatenate([[0], np.cumsum(batch.counts)]).astype(np.int32)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    out = sc.screen(up(batch.frac), up(batch.lattice), up(off), up(batch.types) if with_types else None, crit)
    return sc.metrics_to_numpy(out)


def assert_bit_for_bit(got, want, what):
    for k in REALS:
        g, w = np.asarray(got[k]), getattr(want, k)
        assert g.dtype == np.float32 and w.dtype == np.float32
        both_nan = np.isnan(g) & np.isnan(w)  # (one NaN: the kernel's and numpy's quiet NaN need not share a payload)
        same = g.view(np.uint32) == w.view(np.uint32)
        bad = np.nonzero(~(same | both_nan))[0]
        assert bad.size == 0, f"{what}: {k} differs at crystals {bad[:8].tolist()}: {g[bad[:8]]} vs {w[bad[:8]]}"
    for k in INTS:
        g, w = np.asarray(got[k]), getattr(want, k)
        assert g.dtype == np.int32 and g.shape == w.shape
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {k} differs at crystals {bad[:8].tolist()}: {g[bad[:8]].tolist()} vs {w[bad[:8]].tolist()}"
    assert np.asarray(got["valid"]).tolist() == want.valid.tolist(), what


@pytest.fixture(scope="module")
def random_set():
    return cases.random_set()[0]


def test_kernel_matches_the_f32_restatement_on_the_random_set(dev, random_set):
    crit = cases.criteria()
    for b in random_set:
        assert_bit_for_bit(run_kernel(dev, b, crit), sc.screen_reference_f32(b.frac, b.lattice, b.counts, b.types, crit), b.name)
    b = random_set[-1]  # without species: no MASKED
    got = run_kernel(dev, b, crit, with_types=False)
    assert_bit_for_bit(got, sc.screen_reference_f32(b.frac, b.lattice, b.counts, None, crit), b.name + " without types")
    assert not (got["flags"] & sc.MASKED).any()
    tight = sc.ScreenCriteria(min_distance=1.1, min_volume=150.0, search_radius=2.0, mask_type=2, max_shells=2)  # other thresholds
    assert_bit_for_bit(run_kernel(dev, b, tight), sc.screen_reference_f32(b.frac, b.lattice, b.counts, b.types, tight), b.name + " tight")


@pytest.mark.parametrize("case", cases.hand_cases(), ids=lambda c: c.name)
def test_kernel_on_the_hand_made_cases(dev, case):
    crit = cases.criteria()
    got = run_kernel(dev, case, crit)
    assert_bit_for_bit(got, sc.screen_reference_f32(case.frac, case.lattice, case.counts, case.types, crit), case.name)
    assert got["flags"].tolist() == list(case.expect["flags"])
    assert [tuple(p) for p in got["pair"].tolist()] == list(case.expect["pair"])
    if "min_distance" in case.expect:
        assert got["min_distance"].tolist() == list(case.expect["min_distance"])


def test_kernel_above_the_staging_limit_and_on_1024_crystals(dev):
    crit = cases.criteria()
    big = cases.large_crystal()
    assert max(big.counts) > sc.STAGED_ATOMS
    assert_bit_for_bit(run_kernel(dev, big, crit), sc.screen_reference_f32(big.frac, big.lattice, big.counts, big.types, crit), "large")
    many = cases.many_crystals()
    assert len(many.counts) == 1024
    got = run_kernel(dev, many, crit)
    assert_bit_for_bit(got, sc.screen_reference_f32(many.frac, many.lattice, many.counts, many.types, crit), "many")
    seen = int(np.bitwise_or.reduce(got["flags"]))
    assert seen & sc.CLOSE and seen & sc.MASKED and seen & sc.BEYOND and (got["flags"] == 0).any()


def test_kernel_within_the_derived_bound_of_the_f64_restatement(dev, random_set):
    """Distances within screening.distance_bound (derived in the module docstring of screening.py); integer outputs equal on
    the random set, which is drawn so that they must be.  BEYOND crystals against the same image range, as in the CPU test."""
    crit = cases.criteria()
    for b in list(random_set) + cases.hand_cases() + [cases.large_crystal()]:
        got = run_kernel(dev, b, crit)
        r64 = sc.screen_reference_f64(b.frac, b.lattice, b.counts, b.types, crit, details=True)
        same = sc.screen_reference_f64(b.frac, b.lattice, b.counts, b.types, crit, widen=0)
        assert got["flags"].tolist() == r64.flags.tolist() and got["n_close"].tolist() == r64.n_close.tolist(), b.name
        for k in range(len(b.counts)):
            if got["flags"][k] & (sc.CELL | sc.NONFINITE):
                assert np.isnan(got["min_distance"][k])
                continue
            ref = same if got["flags"][k] & sc.BEYOND else r64
            diff = abs(float(got["min_distance"][k]) - ref.min_distance[k])
            print(f"{b.name}[{k}]: d {got['min_distance'][k]:.7f} d64 {ref.min_distance[k]:.9f} |diff| {diff:.2e} bound {r64.bound[k]:.2e}")
            assert diff <= r64.bound[k], (b.name, k)
            assert float(got["min_distance"][k]) >= r64.min_distance[k] - r64.bound[k], (b.name, k)
            if b.name.startswith("random"):
                assert got["pair"][k].tolist() == ref.pair[k].tolist(), (b.name, k)
            assert abs(float(got["volume"][k]) - r64.volume[k]) <= 1e-5 * r64.volume[k]


def test_argument_errors(dev):
    L = _hip.lib()
    f32 = dict(device=dev, dtype=torch.float32)
    frac, lat, off = torch.rand(3, 3, **f32), torch.eye(3, **f32)[None] * 5, torch.tensor([0, 3], device=dev, dtype=torch.int32)
    out = {k: torch.zeros((1, 5) if k == "pair" else 1, device=dev, dtype=torch.float32 if k in REALS else torch.int32)
           for k in sc.METRIC_KEYS}
    res = _hip.ScreenResultC(*[_hip.ptr(out[k]).value for k in sc.METRIC_KEYS])

    def call(crit=(0.5, 0.1, 3.0, -1, 8), frac=frac, lat=lat, off=off, B=1, N=3, res=res, null_crit=False):
        c = _hip.ScreenCriteriaC(*crit)
        return L.arreau_crystal_screen(_hip.ptr(frac), None, _hip.ptr(lat), _hip.ptr(off), B, N, None if null_crit else ctypes.byref(c),
                                       ctypes.byref(res) if res is not None else None, _hip.stream_ptr(dev))
    assert call() == 0
    for kw, word in [(dict(crit=(-0.5, 0.1, 3.0, -1, 8)), "min_distance"), (dict(crit=(0.5, float("nan"), 3.0, -1, 8)), "min_volume"),
                     (dict(crit=(0.5, 0.1, 0.4, -1, 8)), "search_radius"), (dict(crit=(0.5, 0.1, float("inf"), -1, 8)), "search_radius"),
                     (dict(crit=(0.5, 0.1, 3.0, -1, 9)), "max_shells"), (dict(crit=(0.5, 0.1, 3.0, -1, 0)), "max_shells"),
                     (dict(crit=(0.5, 0.1, 3.0, -2, 8)), "mask_type"), (dict(null_crit=True), "null"), (dict(res=None), "null"),
                     (dict(B=-1), "size"), (dict(lat=None), "null pointer"), (dict(off=None), "null pointer"), (dict(frac=None), "null pointer"),
                     (dict(res=_hip.ScreenResultC(*[_hip.ptr(out[k]).value if k != "pair" else None for k in sc.METRIC_KEYS])), "result array")]:
        assert call(**kw) == -1, kw
        assert word in L.arreau_last_error().decode(), (kw, L.arreau_last_error().decode())
    assert call(B=0, N=0, lat=None, off=None, frac=None) == 0  # an empty batch launches nothing
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="offsets"):
        sc.screen(frac, lat, off.long())


# ------------------------------------------------------------------------------------------------------------ the sampler
def _screen_again(dev, m, res, crit):
    """A separate screen of a returned state: its float32 arrays uploaded again, species as class indices."""
    zs = [int(z) for z in m.z_table_zs.tolist()]
    types = np.array([zs.index(int(z)) for z in res.atomic_numbers], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(res.num_atoms)]).astype(np.int32)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return sc.metrics_to_numpy(sc.screen(up(res.frac_x.astype(np.float32)), up(res.lattice.astype(np.float32)), up(off), up(types), crit))


def _spec():
    from arreau_amd.diffusion import symmetry
    return symmetry.SymmetrySpec.general_positions(["-x,-y,-z"], 3, "triclinic")


SAMPLER_CASES = {
    "philox": dict(noise="philox", max_steps=8), "philox-graph": dict(noise="philox", max_steps=8, use_graph=True),
    "reference": dict(noise="reference", max_steps=6), "device": dict(noise="device", max_steps=6),
    "schedule": dict(num_steps=12), "lattice-system": dict(num_steps=10, lattice_system="hexagonal"),
    "symmetry": dict(num_steps=10, symmetry="spec"), "corrected-resampled": dict(num_steps=8, corrector_steps=1, resample_passes=2, jump_length=4),
    "constant-species": dict(num_steps=8, use_constant_atomic_symbols="first"),
}


@pytest.mark.parametrize("mode", list(SAMPLER_CASES))
def test_sample_with_a_screen(dev, fused_model, mode):
    """metrics equal a separate screen of the returned state (bit for bit), and the returned state is bit-identical to the same
    call without a screen."""
    m, _ = fused_model
    kw = dict(SAMPLER_CASES[mode])
    counts, B = [5, 9, 1, 14], 4
    if kw.get("symmetry") == "spec":
        kw["symmetry"], counts, B = _spec(), None, 3
    if kw.get("use_constant_atomic_symbols") == "first":
        from arreau_amd.diffusion.tools.atomic_number_table import SYMBOL_TO_Z
        symbol = {z: name for name, z in SYMBOL_TO_Z.items()}
        kw["use_constant_atomic_symbols"], counts = [symbol[int(m.z_table_zs[1])]] * 6, 6
    out = []
    for screen in (None, True):
        torch.manual_seed(11)
        np.random.seed(11)
        if kw.get("noise") == "device":
            torch.cuda.manual_seed(11)
        out.append(m.sample(counts, B, seed=99, screen=screen, **kw))
    plain, screened = out
    assert plain.metrics is None and screened.metrics is not None
    for k in ("frac_x", "atomic_numbers", "lattice", "num_atoms"):
        a, b = np.asarray(getattr(plain, k)), np.asarray(getattr(screened, k))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (mode, k)
    mask = -1 if "use_constant_atomic_symbols" in kw else S - 1
    again = _screen_again(dev, m, screened, sc.ScreenCriteria(mask_type=mask))
    assert set(screened.metrics) == set(again) == set(sc.METRIC_KEYS) | {"valid"}
    for k, v in again.items():
        g = np.asarray(screened.metrics[k])
        assert g.dtype == v.dtype and g.shape == v.shape and g.shape[0] == B, (mode, k)
        assert g.tobytes() == v.tobytes(), (mode, k, g, v)
    assert screened.metrics["valid"].tolist() == ((screened.metrics["flags"] & 15) == 0).tolist()
    # the species check follows the state: a crystal has MASKED exactly when one of its atoms is still the mask state (2001)
    first = np.concatenate([[0], np.cumsum(screened.num_atoms)])
    has_mask = [bool((screened.atomic_numbers[first[b]:first[b + 1]] == 2001).any()) for b in range(B)]
    flagged = ((screened.metrics["flags"] & sc.MASKED) != 0).tolist()
    assert flagged == ([False] * B if mask < 0 else [h and not (screened.metrics["flags"][b] & sc.NONFINITE) for b, h in enumerate(has_mask)])


def test_sample_with_criteria_of_its_own(dev, fused_model):
    m, _ = fused_model
    crit = sc.ScreenCriteria(min_distance=1.5, min_volume=40.0, search_radius=4.0, mask_type=-1)
    torch.manual_seed(3)
    np.random.seed(3)
    res = m.sample([6, 3], 2, seed=5, num_steps=8, screen=crit)
    again = _screen_again(dev, m, res, crit)
    for k, v in again.items():
        assert np.asarray(res.metrics[k]).tobytes() == v.tobytes(), k
    assert not (res.metrics["flags"] & sc.MASKED).any()
    with pytest.raises(ValueError, match="screen must be"):
        m.sample([6, 3], 2, seed=5, num_steps=8, screen="yes")


# ------------------------------------------------------------------------------------------------------------ the drivers
def _run(argv, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def _summary(stdout, who):
    m = re.search(rf"screen {who}: accepted (\d+) / attempted (\d+); NONFINITE (\d+), CELL (\d+), CLOSE (\d+), MASKED (\d+), BEYOND (\d+)", stdout)
    assert m, stdout
    return [int(v) for v in m.groups()]


def test_generate_require_valid_and_the_screen_command(dev, tmp_path):
    """--require_valid on one device returns valid crystals only, with a summary that adds up; --screen alone stores the metrics
    of every crystal; python -m arreau_amd.screen finds the same flags in the written file.  The thresholds are loose enough
    for the untrained synthetic model to pass now and then (its species mostly leave the mask state in 30 steps)."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    common = ["--model_path", ckpt, "--num_atoms", "3", "--batch", "16", "--num_steps", "30", "--seed", "5", "--min_distance", "0.05",
              "--min_volume", "0.001"]
    out = str(tmp_path / "valid" / "crystals.npz")
    stdout = _run(["arreau_amd.generate"] + common + ["--num_crystals", "12", "--require_valid", "--max_rounds", "6", "--out", out], tmp_path)
    res = load_sample_results_from_hdf5(out)
    accepted, attempted, *per_flag = _summary(stdout, "total")
    assert _summary(stdout, "rank 0") == [accepted, attempted] + per_flag
    assert res.metrics is not None and res.metrics["valid"].all() and ((res.metrics["flags"] & 15) == 0).all()
    assert len(res.num_atoms) == accepted <= 12 and attempted >= accepted and res.frac_x.shape == (3 * accepted, 3)
    assert accepted == 12 or "short by" in stdout
    assert accepted > 0, stdout  # (the thresholds above were chosen so that the run has something to return)
    # every returned crystal passes a screen of its own from the file
    again = sc.screen_sample_result(res, sc.ScreenCriteria(min_distance=0.05, min_volume=0.001), dev)
    assert again["valid"].all() and again["flags"].tolist() == res.metrics["flags"].tolist()
    # the same seed gives the same file
    out2 = str(tmp_path / "valid2" / "crystals.npz")
    _run(["arreau_amd.generate"] + common + ["--num_crystals", "12", "--require_valid", "--max_rounds", "6", "--out", out2], tmp_path)
    with np.load(out) as a, np.load(out2) as b:
        assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    # --screen alone: every crystal kept, metrics stored, the summary counts them
    out3 = str(tmp_path / "all" / "crystals.npz")
    stdout = _run(["arreau_amd.generate"] + common + ["--num_crystals", "20", "--screen", "--out", out3], tmp_path)
    res3 = load_sample_results_from_hdf5(out3)
    accepted, attempted, *per_flag = _summary(stdout, "total")
    assert attempted == 20 == len(res3.num_atoms) and accepted == int(res3.metrics["valid"].sum())
    assert per_flag == [int(((res3.metrics["flags"] & bit) != 0).sum()) for bit, _ in sc.FLAG_NAMES]
    # without --screen: today's keys
    out4 = str(tmp_path / "plain" / "crystals.npz")
    stdout = _run(["arreau_amd.generate"] + common[:10] + ["--num_crystals", "4", "--out", out4], tmp_path)
    with np.load(out4) as z:
        assert sorted(z.files) == ["atomic_numbers", "frac_x", "idx_start", "lattice", "num_atoms"] and "screen" not in stdout
    # the screen command on the stored file
    out5 = str(tmp_path / "rescreened.npz")
    stdout = _run(["arreau_amd.screen", out3, "--min_distance", "0.05", "--min_volume", "0.001", "--out", out5], tmp_path)
    assert _summary(stdout, "total") == [accepted, attempted] + per_flag
    assert load_sample_results_from_hdf5(out5).metrics["flags"].tolist() == res3.metrics["flags"].tolist()
