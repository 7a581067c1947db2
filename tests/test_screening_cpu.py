"""The structural screen without a GPU: criteria validation, the float32 restatement of the kernel against the float64
restatement, the hand-made cases, the refill driver with a fake sampler, and the file round trip.

The distance bound is screening.distance_bound: derived from the operation order in the module docstring of
arreau_amd/diffusion/screening.py (32 * 2^-24 * the magnitude of the positions and shifts involved), not tuned to any result."""
import argparse
import warnings

import numpy as np
import pytest

from arreau_amd.diffusion import screening as sc
from arreau_amd.diffusion.diffusion_loss import SampleResult
from tests import screening_cases as cases


# --------------------------------------------------------------------------------------------------------------- criteria
def test_criteria_defaults_and_validation():
    c = sc.ScreenCriteria()
    assert (c.min_distance, c.min_volume, c.search_radius, c.mask_type, c.max_shells) == (0.5, 0.1, 3.0, None, 8)
    assert c.with_mask_type(88).mask_type == 88 and sc.ScreenCriteria(mask_type=-1).with_mask_type(88).mask_type == -1
    for kwargs, word in [(dict(min_distance=-0.1), "min_distance"), (dict(min_distance=float("nan")), "min_distance"),
                         (dict(min_volume=float("inf")), "min_volume"), (dict(min_volume="1"), "min_volume"),
                         (dict(search_radius=0.0, min_distance=0.0), "search_radius"), (dict(search_radius=0.4), "at least min_distance"),
                         (dict(mask_type=-2), "mask_type"), (dict(mask_type=1.5), "mask_type"), (dict(max_shells=0), "max_shells"),
                         (dict(max_shells=9), "max_shells"), (dict(max_shells=True), "max_shells")]:
        with pytest.raises(ValueError, match=word):
            sc.ScreenCriteria(**kwargs)
    assert sc.resolve(None) is None and sc.resolve(True) == sc.ScreenCriteria() and sc.resolve(c) is c
    with pytest.raises(ValueError, match="screen must be"):
        sc.resolve("yes")


def test_flag_constants_and_describe():
    assert (sc.NONFINITE, sc.CELL, sc.CLOSE, sc.MASKED, sc.BEYOND, sc.INVALID_MASK) == (1, 2, 4, 8, 16, 15)
    assert sc.describe(0) == "valid" and sc.describe(16) == "valid (BEYOND)" and sc.describe(12) == "CLOSE|MASKED"
    assert sc.describe(20) == "CLOSE|BEYOND" and sc.describe(1) == "NONFINITE"
    assert list(sc.is_valid([0, 16, 4, 24, 2, 1])) == [True, True, False, False, False, False]


def test_header_states_the_same_constants():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "arreau_hip.h")).read()
    get = lambda name: int(re.search(rf"#define ARREAU_SCREEN_{name} (\d+)", text).group(1))
    assert [get(n) for n in ("NONFINITE", "CELL", "CLOSE", "MASKED", "BEYOND", "INVALID_MASK", "MAX_SHELLS")] == \
        [sc.NONFINITE, sc.CELL, sc.CLOSE, sc.MASKED, sc.BEYOND, sc.INVALID_MASK, sc.MAX_SHELLS]


# ------------------------------------------------------------------------------------------- float32 against float64
@pytest.fixture(scope="module")
def random_set():
    return cases.random_set()


def test_random_set_needed_few_replacements(random_set):
    batches, replaced, total = random_set
    assert total == sum(cases.BATCH_SIZES) and sum(len(b.counts) for b in batches) == total
    assert replaced <= 0.05 * total, f"{replaced} of {total} crystals were drawn again"
    atoms = [n for b in batches for n in b.counts]
    assert min(atoms) >= 1 and max(atoms) <= 64 and len(set(atoms)) > 10  # ragged


def test_f32_restatement_agrees_with_f64_on_random_cells(random_set):
    """Distances within the derived bound; pair, n_close and flags identical.  A crystal flagged BEYOND has no contact inside
    the range the rule guarantees, so its reported minimum belongs to the enumerated images: it is compared with the float64
    restatement on the SAME range (widen=0), and against the widened range only as what the rule calls it, an upper bound."""
    crit = cases.criteria()
    seen = 0
    for b in random_set[0]:
        r32 = sc.screen_reference_f32(b.frac, b.lattice, b.counts, b.types, crit)
        r64 = sc.screen_reference_f64(b.frac, b.lattice, b.counts, b.types, crit, details=True)
        same = sc.screen_reference_f64(b.frac, b.lattice, b.counts, b.types, crit, widen=0)
        assert r32.flags.tolist() == r64.flags.tolist(), b.name
        assert r32.n_close.tolist() == r64.n_close.tolist(), b.name
        seen |= int(np.bitwise_or.reduce(r32.flags))
        for k in range(len(b.counts)):
            what = f"{b.name}[{k}] flags {sc.describe(r32.flags[k])}"
            if r32.flags[k] & (sc.CELL | sc.NONFINITE):
                assert np.isnan(r32.min_distance[k]) and (r32.pair[k] == -1).all(), what
                continue
            bound = r64.bound[k]
            ref = same if r32.flags[k] & sc.BEYOND else r64
            print(f"{what}: d32 {r32.min_distance[k]:.7f} d64 {ref.min_distance[k]:.9f} |diff| "
                  f"{abs(r32.min_distance[k] - ref.min_distance[k]):.2e} bound {bound:.2e}")
            assert abs(float(r32.min_distance[k]) - ref.min_distance[k]) <= bound, what
            assert r32.pair[k].tolist() == ref.pair[k].tolist(), what
            assert float(r32.min_distance[k]) >= r64.min_distance[k] - bound, what  # never below the wider search
            assert abs(float(r32.volume[k]) - r64.volume[k]) <= 1e-5 * r64.volume[k], what
            assert abs(float(r32.number_density[k]) - r64.number_density[k]) <= 1e-5 * r64.number_density[k], what
    assert seen & sc.CLOSE and seen & sc.MASKED, "the random set should exercise CLOSE and MASKED"


def test_bound_is_the_documented_multiple_of_the_unit_roundoff():
    L = np.array([[4, 0, 0], [7.5, 1, 0], [0, 0, 6]])
    # G = max over columns of sum_k (1 + n_k) |L_kd| with n = (6, 3, 1): column 0 gives 7 * 4 + 4 * 7.5 = 58
    assert sc.distance_bound(L, (6, 3, 1)) == 32 * 2.0 ** -24 * 58.0


# ------------------------------------------------------------------------------------------------------ hand-made cases
@pytest.mark.parametrize("case", cases.hand_cases(), ids=lambda c: c.name)
def test_hand_made_cases(case):
    crit = cases.criteria()
    r32 = sc.screen_reference_f32(case.frac, case.lattice, case.counts, case.types, crit)
    r64 = sc.screen_reference_f64(case.frac, case.lattice, case.counts, case.types, crit, details=True)
    e = case.expect
    assert r32.flags.tolist() == list(e["flags"]) == r64.flags.tolist()
    assert r32.valid.tolist() == [f & 15 == 0 for f in e["flags"]]
    assert r32.n_close.tolist() == list(e["n_close"]) == r64.n_close.tolist()
    assert [tuple(p) for p in r32.pair.tolist()] == list(e["pair"])
    if e.get("nan_distance"):
        assert np.isnan(r32.min_distance).all() and np.isnan(r64.min_distance).all()
        assert np.isnan(r32.volume).all() == bool(e.get("nan_volume"))
        return
    if "min_distance" in e:
        assert r32.min_distance.tolist() == list(e["min_distance"])  # exact
    for k in range(len(case.counts)):
        assert abs(float(r32.min_distance[k]) - r64.min_distance[k]) <= r64.bound[k]
        if "approx_distance" in e:
            assert abs(r64.min_distance[k] - e["approx_distance"][k]) <= 1e-6


def test_skewed_cell_contact_lies_outside_the_27_images():
    """What the sampling step's neighbour enumeration (shifts -1..1) would report for the skewed hand-made case."""
    L = cases.SKEWED_CELL.astype(np.float64)
    g = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = np.linalg.norm(g[np.any(g != 0, axis=1)] @ L, axis=1)
    assert abs(d.min() - np.hypot(3.5, 1.0)) < 1e-12 and d.min() > 3.6  # about 3.64 A
    r = sc.screen_reference_f32([[0.3, 0.2, 0.1]], [cases.SKEWED_CELL], [1])
    assert abs(float(r.min_distance[0]) - np.sqrt(1.25)) < 1e-6 and max(abs(v) for v in r.pair[0][2:]) == 2


def test_screen_without_gpu_fails_loudly():
    import torch
    from arreau_amd import _hip
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_hip.ArreauHipError):
        sc.screen(torch.zeros(1, 3), torch.eye(3)[None], torch.tensor([0, 1], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------- the refill driver
class FakeSampler:
    """sample_fn of generate_valid_crystals: crystal number c of this sampler (counted over its calls) is valid unless
    c % 3 == 1 (flag CLOSE) or c % 7 == 3 (flag MASKED); its lattice carries (tag, c) so the order can be checked."""

    def __init__(self, tag, always_invalid=False):
        self.tag, self.count, self.calls, self.always_invalid = tag, 0, [], always_invalid

    def __call__(self, n, b):
        self.calls.append(b)
        c = np.arange(self.count, self.count + b)
        self.count += b
        flags = np.where(c % 3 == 1, sc.CLOSE, 0) | np.where(c % 7 == 3, sc.MASKED, 0) | np.where(c % 5 == 0, sc.BEYOND, 0)
        if self.always_invalid:
            flags = flags | sc.CELL
        lattice = np.zeros((b, 3, 3))
        lattice[:, 0, 0], lattice[:, 1, 1] = self.tag, c
        metrics = {"min_distance": c.astype(np.float32), "pair": np.zeros((b, 5), np.int32), "n_close": np.zeros(b, np.int32),
                   "volume": np.ones(b, np.float32), "number_density": np.ones(b, np.float32), "flags": flags.astype(np.int32),
                   "valid": sc.is_valid(flags)}
        return SampleResult(frac_x=np.repeat(c, n)[:, None] * np.ones((1, 3)), atomic_numbers=np.full(b * n, 6.0), lattice=lattice,
                            num_atoms=np.full(b, n, dtype=np.int64), idx_start=np.arange(b) * n, metrics=metrics)


def _valid_numbers(upto):
    return [c for c in range(upto) if c % 3 != 1 and c % 7 != 3]


def test_generate_valid_crystals_refills_in_order():
    from arreau_amd.generate import generate_valid_crystals
    fake = FakeSampler(7)
    res = generate_valid_crystals(fake, 10, 2, num_crystals_per_batch=4)
    # round 1 asks for 10 (4 + 4 + 2): crystals 0..9, valid 0 2 5 6 8 9; round 2 asks for 4: 10..13, valid 11 12; round 3 for 2: 14, 15
    assert fake.calls == [4, 4, 2, 4, 2]
    assert res.lattice[:, 1, 1].tolist() == [0, 2, 5, 6, 8, 9, 11, 12, 14, 15] == _valid_numbers(16)[:10]
    assert res.metrics["valid"].all() and res.metrics["min_distance"].tolist() == res.lattice[:, 1, 1].tolist()
    assert res.frac_x[:, 0].tolist() == np.repeat(res.lattice[:, 1, 1], 2).tolist() and res.idx_start.tolist() == list(range(0, 20, 2))
    st, = res.info["screen_stats"]
    assert (st["attempted"], st["accepted"], st["requested"], st["rounds"], st["rank"]) == (16, 10, 10, 3, 0)
    assert st["flags"] == {"NONFINITE": 0, "CELL": 0, "CLOSE": 5, "MASKED": 2, "BEYOND": 4}


def test_generate_valid_crystals_reports_a_shortfall():
    from arreau_amd.generate import generate_valid_crystals
    fake = FakeSampler(1)
    with pytest.warns(UserWarning, match="2 short"):
        res = generate_valid_crystals(fake, 10, 1, num_crystals_per_batch=256, max_rounds=2)
    assert fake.calls == [10, 4] and len(res.num_atoms) == 8  # not padded
    st, = res.info["screen_stats"]
    assert (st["attempted"], st["accepted"], st["requested"], st["rounds"]) == (14, 8, 10, 2)
    lines = sc.summary_lines(res.info["screen_stats"])
    assert lines[0].startswith("screen rank 0: accepted 8 / attempted 14;") and "short by 2" in lines[0] and lines[-1].startswith("screen total:")
    with pytest.warns(UserWarning):
        none = generate_valid_crystals(FakeSampler(1, always_invalid=True), 3, 1, max_rounds=3)
    assert len(none.num_atoms) == 0 and none.info["screen_stats"][0]["attempted"] == 9
    with pytest.raises(ValueError, match="max_rounds"):
        generate_valid_crystals(fake, 3, 1, max_rounds=0)
    with pytest.raises(ValueError, match="metrics"):
        generate_valid_crystals(lambda n, b: SampleResult(num_atoms=np.ones(b, np.int64)), 3, 1)


def test_generate_valid_crystals_shards_are_independent():
    """Ranks 0..3 of a world of four: each fills its own slice from its own sampler, whatever the others do; rank 0's gather is
    the concatenation in rank order with one statistics entry per rank."""
    from arreau_amd.generate import generate_valid_crystals, shard_range
    alone = {}
    for rank in range(4):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            alone[rank] = generate_valid_crystals(FakeSampler(rank), 10, 1, num_crystals_per_batch=2, rank=rank, world_size=4,
                                                  gather=lambda obj: [obj])  # (a gather that returns this rank alone)
    for rank in range(4):
        res = alone[rank] if rank == 0 else None
        part = generate_valid_crystals(FakeSampler(rank), 10, 1, num_crystals_per_batch=2, rank=rank, world_size=4,
                                       gather=lambda obj, r=rank: [obj] if r == 0 else None)
        if rank == 0:
            start, stop = shard_range(10, 4, 0)
            assert len(res.num_atoms) == stop - start and (res.lattice[:, 0, 0] == 0).all()
            assert part.lattice.tolist() == res.lattice.tolist()
    parts = []
    for rank in range(4):
        generate_valid_crystals(FakeSampler(rank), 10, 1, num_crystals_per_batch=2, rank=rank, world_size=4,
                                gather=lambda obj: parts.append(obj) or [obj])
    whole = generate_valid_crystals(FakeSampler(0), 10, 1, num_crystals_per_batch=2, rank=0, world_size=4, gather=lambda obj: parts)
    assert len(parts) == 4
    assert whole.lattice[:, 0, 0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 3, 3]  # shard sizes 3, 3, 2, 2 in rank order
    assert whole.lattice[:, 1, 1].tolist() == [0, 2, 5, 0, 2, 5, 0, 2, 0, 2]  # every rank's own first valid crystals
    assert [st["rank"] for st in whole.info["screen_stats"]] == [0, 1, 2, 3] and whole.metrics["valid"].all()
    assert sc.total_stats(whole.info["screen_stats"])["accepted"] == 10


def test_generate_rejects_require_valid_with_a_template():
    from arreau_amd.generate import build_parser, check_screen_arguments

    class Stop(Exception):
        pass

    def error(msg):
        raise Stop(msg)
    ap = build_parser()
    args = ap.parse_args(["--model_path", "m.ckpt", "--require_valid", "--template", "t.npz"])
    with pytest.raises(Stop, match="--template"):
        check_screen_arguments(args, error)
    args = ap.parse_args(["--model_path", "m.ckpt", "--require_valid", "--min_distance", "0.7", "--max_rounds", "3"])
    crit = check_screen_arguments(args, error)
    assert crit == sc.ScreenCriteria(min_distance=0.7) and args.max_rounds == 3
    assert check_screen_arguments(ap.parse_args(["--model_path", "m.ckpt"]), error) is None
    assert check_screen_arguments(ap.parse_args(["--model_path", "m.ckpt", "--screen", "--template", "t.npz"]), error) == sc.ScreenCriteria()
    with pytest.raises(Stop, match="search_radius"):
        check_screen_arguments(ap.parse_args(["--model_path", "m.ckpt", "--screen", "--search_radius", "0.2"]), error)
    with pytest.raises(Stop, match="max_rounds"):
        check_screen_arguments(ap.parse_args(["--model_path", "m.ckpt", "--require_valid", "--max_rounds", "0"]), error)
    assert isinstance(ap, argparse.ArgumentParser)


# ----------------------------------------------------------------------------------------------------- file round trip
def test_file_round_trip_with_and_without_metrics(tmp_path):
    from arreau_amd.diffusion.inference.process_generated_crystals import KEYS, load_sample_results_from_hdf5, save_sample_results_to_hdf5
    res = FakeSampler(3)(2, 5)
    plain = SampleResult(frac_x=res.frac_x, atomic_numbers=res.atomic_numbers, lattice=res.lattice, idx_start=res.idx_start,
                         num_atoms=res.num_atoms)
    f0 = save_sample_results_to_hdf5(plain, str(tmp_path / "plain.npz"))
    with np.load(f0) as z:
        assert sorted(z.files) == sorted(KEYS) == sorted(["frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms"])
    back = load_sample_results_from_hdf5(f0)
    assert back.metrics is None and back.frac_x.tolist() == res.frac_x.tolist()
    f1 = save_sample_results_to_hdf5(res, str(tmp_path / "screened.npz"))
    with np.load(f1) as z:
        assert sorted(z.files) == sorted(list(KEYS) + ["screen_" + k for k in ("min_distance", "pair", "n_close", "volume",
                                                                              "number_density", "flags", "valid")])
        assert {k: z[k].tolist() for k in KEYS} == {k: np.load(f0)[k].tolist() for k in KEYS}  # old readers see what they saw
    back = load_sample_results_from_hdf5(f1)
    assert set(back.metrics) == set(res.metrics)
    for k, v in res.metrics.items():
        assert back.metrics[k].dtype == v.dtype and back.metrics[k].tolist() == v.tolist()
    broken = SampleResult(**{**plain.__dict__, "metrics": {**res.metrics, "flags": res.metrics["flags"][:3]}})
    with pytest.raises(ValueError, match="one entry per crystal"):
        save_sample_results_to_hdf5(broken, str(tmp_path / "broken.npz"))


def test_concat_and_select_carry_metrics():
    from arreau_amd.generate import concat_results, select_crystals
    a, b = FakeSampler(1)(2, 3), FakeSampler(2)(3, 2)
    both = concat_results([a, b])
    assert both.metrics["flags"].tolist() == a.metrics["flags"].tolist() + b.metrics["flags"].tolist()
    assert both.num_atoms.tolist() == [2, 2, 2, 3, 3] and both.idx_start.tolist() == [0, 2, 4, 6, 9]
    b.metrics = None
    assert concat_results([a, b]).metrics is None  # all or nothing
    sel = select_crystals(both, [True, False, False, True, True])
    assert sel.num_atoms.tolist() == [2, 3, 3] and sel.idx_start.tolist() == [0, 2, 5] and sel.frac_x.shape == (8, 3)
    assert sel.lattice[:, 0, 0].tolist() == [1, 2, 2] and sel.metrics["min_distance"].tolist() == [0, 0, 1]
