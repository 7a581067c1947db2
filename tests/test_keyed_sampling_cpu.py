"""Keyed sampling without a GPU (diffusion/keyed.py; rules in include/arreau_hip.h, "keyed sampling"): the stream seeds against
their stated definition, key validation before any work, the driver's slot arithmetic, the file layer and the command line."""
import os
import tempfile

import numpy as np
import pytest
import torch

from arreau_amd import generate as gen
from arreau_amd.diffusion import keyed
from arreau_amd.diffusion.diffusion_loss import SampleResult
from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5

ZT = list(range(5))
M32 = 0xFFFFFFFF


def _philox(counter, key):
    """Philox4x32-10 written out independently of keyed.py (Salmon et al., SC'11: two 32 x 32 -> 64 multiplies per round, the key
    bumped by the Weyl constants)."""
    c, k = [int(v) for v in counter], [int(v) for v in key]
    for _ in range(10):
        hi0, lo0 = divmod(0xD2511F53 * c[0], 2 ** 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c[2], 2 ** 32)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return tuple(c)


# the Random123 known-answer vectors of philox4x32_10 (kat_vectors; the ones tests/test_cabi_exports.py feeds the device)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_python_philox_matches_the_known_answers():
    for counter, key, want in KAT:
        assert keyed.philox4x32_10(counter, key) == want
        assert _philox(counter, key) == want


def test_stream_seed_is_its_stated_definition():
    rng = np.random.RandomState(0)
    pairs = [(5, 1), (6, 0), (0, 0), (2 ** 64 - 1, 2 ** 63 - 1), (3, 2 ** 40 + 17)]
    pairs += [(int(rng.randint(0, 2 ** 62)), int(rng.randint(0, 2 ** 62))) for _ in range(20)]
    for seed, key in pairs:
        w = _philox((key & M32, key >> 32, 0x4B455953, 0), (seed & M32, seed >> 32))
        assert keyed.stream_seed(seed, key) == w[0] | (w[1] << 32), (seed, key)
    assert keyed.stream_seed(5, 1) != keyed.stream_seed(6, 0)
    assert keyed.stream_seed(5, 1) != keyed.stream_seed(5 + 1, 1 - 1) and keyed.stream_seed(5, 1) != keyed.stream_seed(1, 5)
    seeds = keyed.stream_seeds(3, range(10000))
    assert seeds.dtype == np.uint64 and len(set(seeds.tolist())) == 10000
    assert int(seeds[4711]) == keyed.stream_seed(3, 4711)


def test_uniforms_and_angle_draws():
    s = keyed.stream_seed(9, 2)
    w = _philox((7, 0, 15, 0), (s & M32, s >> 32))
    assert keyed.raw_words(s, 0, 15, 7) == w
    assert keyed.uniform(s, 0, 15, 7) == (w[0] >> 8) / 2.0 ** 24
    draw = keyed.angle_uniforms(s)
    got = [draw(60, 120) for _ in range(3)]
    assert got == [60 + 60 * keyed.uniform(s, 0, 15, j) for j in range(3)]
    assert all(60 <= a < 120 for a in got)


def test_slot_key():
    assert keyed.slot_key(4, 0, 10) == 4 and keyed.slot_key(4, 3, 10) == 34
    for bad in ((10, 0, 10), (-1, 0, 10), (0, -1, 10)):
        with pytest.raises(ValueError):
            keyed.slot_key(*bad)


# ---------------------------------------------------------------------------------------------------- validation
class NoEngine:
    """A model whose engine must not be asked for: validation comes before any work."""

    def engine(self, *a, **k):
        raise AssertionError("the engine was touched before the keys were validated")


def _dl():
    from types import SimpleNamespace

    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    return DiffusionLoss(SimpleNamespace(radius=5.0, max_neighbors=16, num_timesteps=50), len(ZT))


@pytest.mark.parametrize("kw,match", [
    (dict(crystal_keys=[0, -1], seed=1), "outside"),
    (dict(crystal_keys=[0, 2 ** 63], seed=1), "outside"),
    (dict(crystal_keys=[0, 1, 2], seed=1), "3 keys for a batch of 2"),
    (dict(crystal_keys=[7, 7], seed=1), "twice"),
    (dict(crystal_keys=[0, 1]), "need a seed"),
    (dict(crystal_keys=[0, 1], seed=1, noise="device"), "noise='philox'"),
    (dict(crystal_keys=[0, 1.5], seed=1), "integers"),
])
def test_bad_keys_are_rejected_before_any_work(kw, match):
    torch.manual_seed(3)
    np.random.seed(3)
    t_state, n_state = torch.random.get_rng_state(), np.random.get_state()
    with pytest.raises(ValueError, match=match):
        _dl().sample(model=NoEngine(), z_table=ZT, num_atoms_per_sample=3, num_samples_in_batch=2, **kw)
    assert torch.equal(torch.random.get_rng_state(), t_state)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), n_state))


def test_the_wrapper_rejects_bad_keys_too():
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=12, seed=1, num_timesteps=20)
    m.engine = NoEngine().engine
    t_state = torch.random.get_rng_state()
    for kw in (dict(crystal_keys=[1, 1], seed=2), dict(crystal_keys=[1, 2]), dict(crystal_keys=[1, 2], seed=2, noise="reference"),
               dict(crystal_keys=[1], seed=2)):
        with pytest.raises(ValueError):
            m.sample(3, 2, **kw)
    crystals = SampleResult(frac_x=np.zeros((2, 3)), atomic_numbers=np.ones(2), lattice=np.eye(3)[None] * np.ones((2, 1, 1)) * 4,
                            num_atoms=np.array([1, 1]), idx_start=np.array([0, 1]))
    for kw in (dict(crystal_keys=[1, 1], seed=2), dict(crystal_keys=[1, 2]), dict(crystal_keys=[1, 2, 3], seed=2)):
        with pytest.raises(ValueError):
            m.noise_to(crystals, 5, **kw)
    assert torch.equal(torch.random.get_rng_state(), t_state)


# ---------------------------------------------------------------------------------------------------- the driver
def _valid(key):
    """Validity as a function of the key alone (about a third of the keys fail; key 5 and its retry 17 both fail)."""
    return key not in (5, 17) and keyed.stream_seed(1, key) % 3 != 0


def _fake_sample(log):
    def sample(keys):
        log.append(list(keys))
        ids = np.asarray(keys, dtype=np.int64)
        valid = np.array([_valid(int(k)) for k in keys])
        return SampleResult(frac_x=np.repeat(ids, 2)[:, None] * np.ones((1, 3)) / 1e4, atomic_numbers=np.repeat(1 + ids % 5, 2).astype(float),
                            lattice=ids[:, None, None] * np.eye(3)[None], num_atoms=np.full(len(ids), 2), idx_start=2 * np.arange(len(ids)),
                            metrics=dict(flags=(~valid).astype(np.int64), valid=valid), crystal_keys=ids)
    return sample


def _run_driver(num, world, batch, max_rounds, require_valid=True):
    """Every rank's generate_keyed through a gather that collects them (the ranks do not talk before it)."""
    import warnings
    locals_, logs = [], []
    for rank in range(world):
        log = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gen.generate_keyed(_fake_sample(log), range(num), num, batch, rank, world, gather=lambda obj: locals_.append(obj) or [None],
                               require_valid=require_valid, max_rounds=max_rounds) if world > 1 else \
                locals_.append(gen.generate_keyed(_fake_sample(log), range(num), num, batch, 0, 1, require_valid=require_valid,
                                                  max_rounds=max_rounds))
        logs.append(log)
    return gen.concat_results(locals_), logs


def test_keyed_require_valid_does_not_depend_on_ranks_or_batch():
    num, rounds = 12, 3
    want = {}
    for slot in range(num):  # the stated rule: the first valid attempt a < rounds, key a * num + slot
        ok = [a for a in range(rounds) if _valid(a * num + slot)]
        if ok:
            want[slot] = ok[0] * num + slot
    assert 5 not in want or want[5] == 29  # (slot 5: attempts 0 and 1 fail by construction)
    assert any(k >= num for k in want.values()) and len(want) <= num
    ref = None
    for world in (1, 2, 3):
        for batch in (2, 5, 256):
            res, logs = _run_driver(num, world, batch, rounds)
            keys = res.crystal_keys.tolist()
            assert {k % num: k for k in keys} == want, (world, batch)
            assert [k % num for k in keys] == sorted(want), "slot order"
            assert all(len(part) <= batch for log in logs for part in log)
            # only open slots are retried: no key is sampled twice, no slot is retried after it was accepted
            tried = [k for log in logs for part in log for k in part]
            assert len(tried) == len(set(tried))
            assert all(not any(t % num == s and t > k for t in tried) for s, k in want.items())
            arrays = (res.frac_x, res.atomic_numbers, res.lattice, res.num_atoms, res.idx_start, res.crystal_keys)
            if ref is None:
                ref = arrays
            assert all(np.array_equal(a, b) for a, b in zip(arrays, ref)), (world, batch)
            assert np.array_equal(res.lattice[:, 0, 0], np.asarray(keys, dtype=float))  # the crystal of its key


def test_keyed_shortfall_is_reported_not_padded():
    num = 12
    with pytest.warns(UserWarning, match="short"):
        res = gen.generate_keyed(_fake_sample([]), range(num), num, 4, 0, 1, require_valid=True, max_rounds=1)
    want = [s for s in range(num) if _valid(s)]
    assert res.crystal_keys.tolist() == want and len(want) < num
    st = res.info["screen_stats"][0]
    assert st["requested"] == num and st["rounds"] == 1 and st["accepted"] == len(want) and st["attempted"] == num


def test_keyed_without_screening_and_with_given_slots():
    log = []
    res = gen.generate_keyed(_fake_sample(log), [7, 2], 10, 256, 0, 1)
    assert res.crystal_keys.tolist() == [2, 7] and log == [[7, 2]]
    res, _ = _run_driver(7, 3, 2, 1, require_valid=False)
    assert res.crystal_keys.tolist() == list(range(7))


# ---------------------------------------------------------------------------------------------------- the file layer
def _result(keys=None):
    na = np.array([2, 1, 3])
    return SampleResult(frac_x=np.arange(18.0).reshape(6, 3) / 20, atomic_numbers=np.arange(6.0), lattice=np.arange(27.0).reshape(3, 3, 3),
                        num_atoms=na, idx_start=np.cumsum(na) - na, crystal_keys=keys)


def test_file_round_trip_and_unkeyed_files_are_unchanged():
    with tempfile.TemporaryDirectory() as d:
        keys = np.array([2 ** 62 + 5, 0, 17], dtype=np.int64)
        back = load_sample_results_from_hdf5(save_sample_results_to_hdf5(_result(keys), os.path.join(d, "k.npz")))
        assert back.crystal_keys.dtype == np.int64 and np.array_equal(back.crystal_keys, keys)
        plain = save_sample_results_to_hdf5(_result(), os.path.join(d, "p.npz"))
        with np.load(plain) as z:
            assert z.files == ["frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms"]
        assert load_sample_results_from_hdf5(plain).crystal_keys is None
        with pytest.raises(ValueError):
            save_sample_results_to_hdf5(_result(np.array([1, 2])), os.path.join(d, "bad.npz"))
    # concat / select carry the keys; a part without keys drops them
    a, b = _result(np.array([1, 2, 3])), _result(np.array([4, 5, 6]))
    assert gen.concat_results([a, b]).crystal_keys.tolist() == [1, 2, 3, 4, 5, 6]
    assert gen.concat_results([a, _result()]).crystal_keys is None
    assert gen.select_crystals(a, [True, False, True]).crystal_keys.tolist() == [1, 3]
    assert gen.select_crystals(_result(), [True, False, True]).crystal_keys is None


# ---------------------------------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("argv,match", [
    (["--keyed"], "--keyed needs --seed"),
    (["--keyed", "--seed", "3", "--num_crystals", "6", "--keys", "1,6"], "outside 0..5"),
    (["--keyed", "--seed", "3", "--num_crystals", "6", "--keys", "-1"], "outside 0..5"),
    (["--keyed", "--seed", "3", "--num_crystals", "6", "--keys", "2,2"], "twice"),
    (["--seed", "3", "--keys", "1"], "--keys needs --keyed"),
])
def test_command_line_errors(argv, match, capsys):
    ap = gen.build_parser()
    args = ap.parse_args(["--model_path", "none.ckpt"] + argv)
    with pytest.raises(SystemExit):
        gen.check_keyed_arguments(args, ap.error)
    assert match in capsys.readouterr().err


def test_command_line_slots():
    ap = gen.build_parser()
    base = ["--model_path", "none.ckpt", "--seed", "3", "--num_crystals", "6"]
    assert gen.check_keyed_arguments(ap.parse_args(base), ap.error) is None
    assert gen.check_keyed_arguments(ap.parse_args(base + ["--keyed"]), ap.error) == list(range(6))
    assert gen.check_keyed_arguments(ap.parse_args(base + ["--keyed", "--keys", "4, 1"]), ap.error) == [4, 1]


# ---------------------------------------------------------------------------------------------------- main(), its keyed branches
class _FakeModel:
    """Stands in for the loaded checkpoint in generate.main(): crystal b of a call is a function of its key alone (the cell is
    key * I, the positions key / 1e4), and every call is recorded."""

    def __init__(self):
        from types import SimpleNamespace
        self.diffusion_loss = SimpleNamespace(T=50)
        self.calls = []

    def noise_to(self, crystals, t, seed=None, crystal_keys=None):
        self.calls.append(("noise_to", int(t), seed, list(crystal_keys)))
        return ("state", np.asarray(crystals.num_atoms), list(crystal_keys))

    def sample(self, n=None, b=None, *args, condition=None, initial_state=None, seed=None, crystal_keys=None, **kw):
        if initial_state is not None:
            assert initial_state[0] == "state" and initial_state[2] == list(crystal_keys)  # the state noised under the same keys
            na = initial_state[1]
        else:
            na = np.asarray(condition.num_atoms)
        self.calls.append(("sample", seed, list(crystal_keys)))
        ids = np.asarray(crystal_keys, dtype=np.int64)
        assert len(ids) == len(na)
        return SampleResult(frac_x=np.repeat(ids, na)[:, None] * np.ones((1, 3)) / 1e4, atomic_numbers=np.repeat(1.0 + ids % 5, na),
                            lattice=ids[:, None, None] * np.eye(3)[None], num_atoms=na, idx_start=np.cumsum(na) - na,
                            crystal_keys=ids)


def _run_main(monkeypatch, argv):
    import sys

    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    model = _FakeModel()
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.setattr(PONITA_DIFFUSION, "load_from_checkpoint", classmethod(lambda cls, *a, **k: model))
    monkeypatch.setattr(sys, "argv", ["generate"] + argv)
    for var in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ARREAU_GENERATE_GPU_LOCK"):
        monkeypatch.delenv(var, raising=False)
    torch.manual_seed(11)
    np.random.seed(11)
    t_state, n_state = torch.random.get_rng_state(), np.random.get_state()
    gen.main()
    assert torch.equal(torch.random.get_rng_state(), t_state)  # a keyed run seeds and reads no generator
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), n_state))
    return model


def _file_of(d, counts, name):
    na = np.asarray(counts)
    res = SampleResult(frac_x=np.random.RandomState(0).rand(int(na.sum()), 3), atomic_numbers=np.ones(int(na.sum())),
                       lattice=np.eye(3)[None] * 4.0 * np.ones((len(na), 1, 1)), num_atoms=na, idx_start=np.cumsum(na) - na)
    return save_sample_results_to_hdf5(res, os.path.join(d, name))


@pytest.mark.parametrize("batch", [2, 256])
def test_main_keys_a_start_file_by_the_crystal_index(monkeypatch, batch):
    with tempfile.TemporaryDirectory() as d:
        counts = [2, 1, 3, 2, 1]
        out = os.path.join(d, "out.npz")
        model = _run_main(monkeypatch, ["--model_path", "none.ckpt", "--keyed", "--seed", "3", "--start_from", _file_of(d, counts, "start.npz"),
                                        "--start_t", "7", "--batch", str(batch), "--out", out])
        res = load_sample_results_from_hdf5(out)
        assert res.crystal_keys.tolist() == [0, 1, 2, 3, 4] and res.num_atoms.tolist() == counts
        assert np.array_equal(res.lattice[:, 0, 0], np.arange(5.0))
        parts = [[0, 1], [2, 3], [4]] if batch == 2 else [[0, 1, 2, 3, 4]]
        assert [c for c in model.calls if c[0] == "noise_to"] == [("noise_to", 7, 3, p) for p in parts]
        assert [c for c in model.calls if c[0] == "sample"] == [("sample", 3, p) for p in parts]


@pytest.mark.parametrize("batch", [4, 256])
def test_main_keys_tiled_templates_by_file_index_and_copy(monkeypatch, batch):
    with tempfile.TemporaryDirectory() as d:
        counts, K = [2, 1, 3], 2
        out = os.path.join(d, "out.npz")
        model = _run_main(monkeypatch, ["--model_path", "none.ckpt", "--keyed", "--seed", "9", "--template", _file_of(d, counts, "tmpl.npz"),
                                        "--fix", "lattice", "--samples_per_template", str(K), "--batch", str(batch), "--out", out])
        want = [0, 2, 4, 1, 3, 5]  # tiled order t0, t1, t2, t0, t1, t2: index in the file * K + the copy
        assert want == [keyed.template_key(j, 3, K) for j in range(6)]
        res = load_sample_results_from_hdf5(out)
        assert res.crystal_keys.tolist() == want and res.num_atoms.tolist() == counts * K
        parts = [want[:4], want[4:]] if batch == 4 else [want]
        assert model.calls == [("sample", 9, p) for p in parts]
    with pytest.raises(ValueError):
        keyed.template_key(6, 3, 2)
