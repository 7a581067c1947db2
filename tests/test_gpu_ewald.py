"""The Ewald sums on the device (arreau_crystal_ewald, csrc/ewald.hip) on the batches of tests/ewald_cases.py: flags, n_pairs and
n_reciprocal exact against the float32-mode restatement run at the device's own alpha (which first has to agree with the rule to
1e-13); energy, its four parts and the potentials against the float64 restatement within ewald.F32_BOUND -- 16 times the
deviation measured on the CPU by tools/exp/ewald_f32_deviation.py, never from the kernel's output --; every ragged crystal alone,
in the batch and at another place in it bit for bit; one crystal at three alphas; the supercell; sample(ewald=...), the file and
the screen's command line; the argument errors and the export.  Needs an MI355X: `-m gpu`.

Measured on one MI355X (the figures the tests print): the device's largest deviation from float64 per batch equals the float32
mode's to three digits -- 4.50e-6 (energies, `ragged`) and 1.24e-4 (potentials, `large`) at most -- against the bound 1.98e-3; the
table is in DESIGN.md section 7."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import ewald
from tests import ewald_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUN = {}
SAMPLE_CHARGES = {z: (1.0 if z % 2 else -1.0) for z in range(1, S)}  # every species of the synthetic models but the mask state


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, bt):
    off = np.concatenate([[0], np.cumsum(bt.counts)]).astype(np.int32)
    return up(dev, bt.frac.reshape(-1, 3)), up(dev, bt.lattice), up(dev, off), up(dev, cases.charges(bt))


def launch(dev, bt):
    return ewald.result_to_numpy(ewald.ewald(*device_batch(dev, bt), bt.params))


def run(dev, name):
    """The kernel's arrays of one named batch (one launch each, cached)."""
    if name not in _RUN:
        _RUN[name] = launch(dev, cases.batch(name))
    return _RUN[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("name", cases.BATCHES)
def test_counts_and_flags_are_exact(dev, name):
    bt, r = cases.reference(name)
    got = run(dev, name)
    assert set(got) == set(ewald.RESULT_KEYS) and got["potential"].shape == (int(np.sum(bt.counts)),)
    assert got["energy"].dtype == np.float64 and got["n_pairs"].dtype == np.int64 and got["n_reciprocal"].dtype == np.int32 and got["flags"].dtype == np.int32
    ok = (r.flags & ewald.INVALID_MASK) == 0
    assert (r.reciprocal_margin[ok] >= ewald.MARGIN_GUARD).all()  # no crystal is left out of the exact comparison
    assert np.array_equal(got["flags"], r.flags), name
    # the device's alpha is the rule's to an ulp or two of cbrt; the float32 mode then runs at the device's own
    assert not np.isnan(got["alpha"][ok]).any() and (np.abs(got["alpha"][ok] / r.alpha[ok] - 1.0) <= 1e-13).all()
    r32 = ewald.ewald_reference(bt.frac, bt.lattice, bt.counts, cases.charges(bt), bt.params, dtype=np.float32, alpha=got["alpha"])
    assert np.array_equal(got["flags"], r32.flags) and np.array_equal(got["n_pairs"], r32.n_pairs) and np.array_equal(got["n_reciprocal"], r32.n_reciprocal), name
    for k in ewald.CRYSTAL_REALS:
        assert np.isnan(got[k][~ok]).all() and not np.isnan(got[k][ok]).any(), k
    for b in range(len(bt.counts)):
        assert np.isnan(got["potential"][cases.atoms_of(bt, b)]).all() == (not ok[b]) or bt.counts[b] == 0
    assert (np.abs(got["volume"][ok] / r.volume[ok] - 1.0) <= 1e-15).all() and np.array_equal(bits(got["net_charge"][ok]), bits(r.net_charge[ok]))


@pytest.mark.parametrize("name", cases.BATCHES)
def test_energies_and_potentials_match_the_float64_restatement(dev, name):
    bt, r = cases.reference(name)
    got = run(dev, name)
    e_err, p_err = cases.deviation(r, got, bt)
    print(name, "largest deviation from float64: energies", e_err, "potentials", p_err, "bound", ewald.F32_BOUND, "float32 mode", ewald.F32_DEVIATION[name])
    assert e_err <= ewald.F32_BOUND and p_err <= ewald.F32_BOUND, (name, e_err, p_err)
    # E = (1 / 2) sum q potential of the device's own potentials (volts), one rounding per operation in atom order: bit for bit
    q = cases.charges(bt).astype(np.float64)
    for b in np.flatnonzero((r.flags & ewald.INVALID_MASK) == 0):
        total = np.float64(0.0)
        for qa, pa in zip(q[cases.atoms_of(bt, b)], got["potential"][cases.atoms_of(bt, b)]):
            total = total + qa * pa
        assert got["energy"][b] == np.float64(0.5) * total, (name, b)


def test_a_crystal_gives_the_same_bits_alone_in_the_batch_and_elsewhere(dev):
    bt = cases.batch("ragged")
    got = run(dev, "ragged")
    B = len(bt.counts)
    assert B == 70
    crystals = [cases.random_crystal(s) for s in cases.RAGGED_SEEDS]
    turned = launch(dev, cases._batch("turned", crystals[::-1]))  # every crystal at another place: the batch backwards
    for b in range(B):
        alone = launch(dev, cases.single(bt, b))
        for k in ewald.RESULT_KEYS:
            here = got[k][cases.atoms_of(bt, b)] if k == "potential" else got[k][b:b + 1]
            assert np.array_equal(bits(alone[k]), bits(here)), (b, k)
            if k != "potential":
                assert np.array_equal(bits(turned[k][B - 1 - b:B - b]), bits(here)), (b, k)
    first = np.concatenate([[0], np.cumsum(bt.counts[::-1])])
    for b in range(B):  # the potentials of the turned batch, crystal by crystal
        t = B - 1 - b
        assert np.array_equal(bits(turned["potential"][first[t]:first[t + 1]]), bits(got["potential"][cases.atoms_of(bt, b)])), b
    again = launch(dev, bt)  # and a second launch of the whole batch
    for k in ewald.RESULT_KEYS:
        assert np.array_equal(bits(again[k]), bits(got[k])), k
    pair = cases._batch("pair", [cases.random_crystal(3), cases.random_crystal(500, ewald.cb.STAGED_ATOMS + 1)])  # past the staging
    two = launch(dev, pair)
    big = run(dev, "large")
    for k in ewald.RESULT_KEYS:
        assert np.array_equal(bits(two[k][pair.counts[0]:] if k == "potential" else two[k][1:]), bits(big[k])), k


def test_alpha_and_the_supercell_on_the_device(dev):
    """One crystal at alpha 0.6 (three reciprocal rounds), 0.25 and 0.35: two runs agree within twice the bound, on the smaller of
    their two scales (|E_self| and the potential's scale grow with alpha).  The 2 x 1 x 1 supercell per formula unit likewise."""
    runs = [(run(dev, n), cases.reference(n)) for n in ("rounds", "rounds 0.25", "rounds 0.35")]
    for i in range(3):
        for j in range(i + 1, 3):
            (a, (bt, ra)), (b, (_, rb)) = runs[i], runs[j]
            assert a["alpha"][0] != b["alpha"][0] and a["n_reciprocal"][0] != b["n_reciprocal"][0]
            assert abs(a["energy"][0] - b["energy"][0]) <= 2.0 * ewald.F32_BOUND * min(abs(ra.self[0]), abs(rb.self[0]))
            scale = min(cases.potential_scale(ra, bt)[0], cases.potential_scale(rb, bt)[0])
            assert np.abs(a["potential"] - b["potential"]).max() <= 2.0 * ewald.F32_BOUND * scale
    got, (bt, r) = run(dev, "textbook"), cases.reference("textbook")
    one, two = cases.TEXTBOOK_NAMES.index("nacl"), cases.TEXTBOOK_NAMES.index("nacl_doubled")
    assert abs(got["energy"][two] / 8.0 - got["energy"][one] / 4.0) <= 2.0 * ewald.F32_BOUND * min(abs(r.self[two]) / 8.0, abs(r.self[one]) / 4.0)
    assert abs(ewald.madelung(got, one, cases.A_NACL / 2.0, 4) - 1.7475645946) < 1e-5 and got["n_reciprocal"][two] > got["n_reciprocal"][one]


def test_charges_or_atomic_numbers(dev):
    bt = cases.batch("flags")
    frac, lattice, off, q = device_batch(dev, bt)
    by_z = ewald.result_to_numpy(ewald.ewald(frac, lattice, off, up(dev, bt.species.astype(np.int32)), bt.params))
    by_z64 = ewald.result_to_numpy(ewald.ewald(frac, lattice, off, up(dev, bt.species), bt.params))
    from_double = ewald.result_to_numpy(ewald.ewald(frac, lattice, off, q.to(torch.float64), ewald.EwaldParams(alpha=1.0)))
    for k in ewald.RESULT_KEYS:
        for other in (by_z, by_z64, from_double):
            assert np.array_equal(bits(other[k]), bits(run(dev, "flags")[k])), k
    with pytest.raises(ValueError, match="need EwaldParams.charges"):
        ewald.ewald(frac, lattice, off, up(dev, bt.species), ewald.EwaldParams())
    with pytest.raises(ValueError, match="must be a"):
        ewald.ewald(frac, lattice, off, q[:-1], bt.params)
    empty = ewald.ewald(torch.empty((0, 3), device=dev), torch.empty((0, 3, 3), device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                        torch.empty(0, device=dev))
    assert empty["energy"].shape == (0,) and empty["potential"].shape == (0,)  # no crystals at all: nothing is launched


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_sample_with_ewald_the_file_and_the_screen(dev, fused_model, tmp_path):
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import instrument_lines
    m, _ = fused_model
    params = ewald.EwaldParams(charges=SAMPLE_CHARGES, accuracy=1e-6)
    # a gas of a few atoms in a cell of random lengths: a large alpha keeps the images within max_shells, and a charge for the mask
    # state lets the crystals that still hold one be computed
    wide = ewald.EwaldParams(charges={**SAMPLE_CHARGES, cases.MASK_ATOMIC_NUMBER: 1.0}, accuracy=1e-6, alpha=2.0)
    out = []
    for kw in ({}, dict(ewald=None), dict(ewald=params, coordination=True, screen=True), dict(coordination=True, screen=True), dict(ewald=wide)):
        torch.manual_seed(3)
        np.random.seed(3)
        r = m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)
        out.append((r, torch.random.get_rng_state(), np.random.uniform()))
    plain = out[0][0]
    for r, rng, after in out[1:]:
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and np.array_equal(plain.num_atoms, r.num_atoms)
        assert torch.equal(out[0][1], rng) and out[0][2] == after
    none, every, others, full = out[1][0], out[2][0], out[3][0], out[4][0]
    assert plain.ewald is None and none.ewald is None and others.ewald is None and every.xrd is None and full.metrics is None
    for field in ("metrics", "coordination"):  # every other instrument's arrays: as without the keyword
        x, y = getattr(every, field), getattr(others, field)
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))), (field, k)
    starts = np.cumsum(every.num_atoms) - every.num_atoms
    masked = np.array([(np.rint(every.atomic_numbers[a:a + n]) == cases.MASK_ATOMIC_NUMBER).any() for a, n in zip(starts, every.num_atoms)])
    for r, p in ((every, params), (full, wide)):
        c = r.ewald
        assert set(c) == set(ewald.STORED_KEYS) and c["energy"].shape == (3,) and c["potential"].shape == c["charge"].shape == c["species"].shape == (12,)
        direct = ewald.ewald_sample_result(r, p, dev)  # the engine-free entry point on the returned crystals
        for k in ewald.STORED_KEYS:
            assert np.array_equal(bits(c[k]), bits(direct[k])), k
        q = ewald.host_charges(r.atomic_numbers, p)
        assert np.array_equal(bits(c["charge"]), bits(q)) and np.array_equal(c["species"], np.rint(r.atomic_numbers).astype(np.int64))
        ref32 = ewald.ewald_reference(r.frac_x, r.lattice, r.num_atoms, q, p, dtype=np.float32, alpha=c["alpha"])
        assert np.array_equal(c["flags"], ref32.flags) and np.array_equal(c["n_pairs"], ref32.n_pairs)
        ref = ewald.ewald_reference(r.frac_x, r.lattice, r.num_atoms, q, p)
        ok = (ref.flags & ewald.INVALID_MASK) == 0
        assert np.array_equal(c["flags"], ref.flags) and (np.abs(c["energy"][ok] - ref.energy[ok]) <= ewald.F32_BOUND * np.abs(ref.self[ok])).all()
        print("sample(ewald=...): flags", c["flags"].tolist(), "energy per atom", c["energy_per_atom"].tolist())
    c = every.ewald
    assert ((c["flags"] & ewald.INVALID_MASK) != 0)[masked].all() and np.isnan(c["energy_per_atom"][masked]).all()  # no charge for the mask state
    # the file keeps the arrays; the screen's command line gives the same summary and the same arrays from the file
    c, full.idx_start = full.ewald, starts
    assert ((c["flags"] & ewald.INVALID_MASK) == 0).any() and not np.isnan(c["energy_per_atom"]).all()  # the round trip carries numbers
    name, out_name = str(tmp_path / "crystals.npz"), str(tmp_path / "screened.npz")
    back = load_sample_results_from_hdf5(save_sample_results_to_hdf5(full, name))
    for k in ewald.STORED_KEYS:
        assert np.array_equal(bits(back.ewald[k]), bits(c[k])) and back.ewald[k].dtype == c[k].dtype, k
    assert [f for f in np.load(name).files if f.startswith("ewald_")] == ["ewald_" + k for k in ewald.STORED_KEYS]
    text = _child(["arreau_amd.screen", name, "--ewald", "--ewald_charges", ",".join(f"{z}={v:g}" for z, v in wide.charges),
                   "--ewald_accuracy", "1e-6", "--ewald_alpha", "2.0", "--out", out_name], 120)
    lines = [ln for ln in text.splitlines() if ln.startswith("ewald ")]
    assert lines == instrument_lines("ewald", full) and len(lines) == 2 and lines[1].startswith("ewald total: 3 crystals"), text
    stored = load_sample_results_from_hdf5(out_name).ewald
    for k in ewald.STORED_KEYS:
        assert np.array_equal(bits(stored[k]), bits(c[k])), k


def test_argument_errors_touch_nothing(dev):
    bt = cases.single(cases.batch("textbook"), 1)
    frac, lattice, off, q = device_batch(dev, bt)
    with pytest.raises(ValueError, match="ewald: offsets"):
        ewald.ewald(frac, lattice, off.to(torch.int64), q)
    out = ewald.ewald(frac, lattice, off, q, bt.params)
    work = torch.empty_like(out["potential"])
    before = {k: out[k].clone() for k in ewald.RESULT_KEYS}
    r = _hip.EwaldResultC(*[_hip.ptr(out[k]).value for k in ewald.RESULT_KEYS], _hip.ptr(work).value)
    good = (1e-8, 0.0, 8, 64)
    change = lambda i, v: good[:i] + (v,) + good[i + 1:]
    call = _hip.lib().arreau_crystal_ewald
    EINVAL = -1  # ARREAU_EINVAL
    B, N = 1, int(frac.shape[0])
    trials = [(B, N, None, ctypes.byref(r)), (B, N, good, None), (-1, N, good, ctypes.byref(r)), (B, -1, good, ctypes.byref(r)),
              (B, N, good, ctypes.byref(_hip.EwaldResultC()))]
    trials += [(B, N, bad, ctypes.byref(r)) for bad in (
        change(0, 0.0), change(0, 1.0), change(0, -1e-3), change(0, float("nan")), change(1, -0.1), change(1, float("nan")), change(1, float("inf")),
        change(2, 0), change(2, 9), change(3, 0), change(3, 128))]
    args = lambda: (_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), _hip.ptr(q))
    for b, n, p, res in trials:
        c = ctypes.byref(_hip.EwaldParamsC(*p)) if p is not None else None
        assert call(*args(), b, n, c, res, _hip.stream_ptr(dev)) == EINVAL, (b, n, p)
        assert b"arreau_crystal_ewald" in _hip.lib().arreau_last_error()
    c = ctypes.byref(_hip.EwaldParamsC(*good))
    assert call(None, _hip.ptr(lattice), _hip.ptr(off), _hip.ptr(q), B, N, c, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    assert call(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), None, B, N, c, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    one_null = _hip.EwaldResultC(*[_hip.ptr(out[k]).value if k != "self" else None for k in ewald.RESULT_KEYS], _hip.ptr(work).value)
    assert call(*args(), B, N, c, ctypes.byref(one_null), _hip.stream_ptr(dev)) == EINVAL
    assert call(None, None, None, None, 0, 0, c, ctypes.byref(_hip.EwaldResultC()), _hip.stream_ptr(dev)) == 0  # B == 0: OK
    torch.cuda.synchronize()
    for k in ewald.RESULT_KEYS:
        assert torch.equal(before[k], out[k]), k


def test_sample_takes_the_keyword_and_the_symbol_is_exported(fused_model):
    """What fails without the feature: sample(ewald=...) is a TypeError and the entry point is not in the library."""
    import inspect
    m, _ = fused_model
    assert "ewald" in inspect.signature(m.sample).parameters
    assert "arreau_crystal_ewald" in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_ewald")
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_ewald(" in fh.read()
