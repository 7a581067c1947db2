"""Keyed sampling on the GPU (rules in include/arreau_hip.h, "keyed sampling"; diffusion/keyed.py): the keyed draws against their
Python restatement, a crystal's independence of its batch, the keyed loop against its steps, segments, and the default path."""
import os

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import keyed, resampling as rs, respacing
from tests.sampling_helpers import Case, S, T, assert_same_bits, dev, full_i32, fused_model, model_seed  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

COUNTS = [3, 7, 5]
KEYS = [11, 4, 29]
SEED = 20240917
CLIP = 0.999
SNR = 0.16


class Batch(Case):
    COUNTS = COUNTS


def _seeds(dev, seed, keys):
    return torch.as_tensor(keyed.stream_seeds(seed, keys).view(np.int64), device=dev).contiguous()


def _offsets(dev, counts):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)


# -------------------------------------------------------------------------------------------------------------- draws
def _box_muller(words):
    """The normals of raw words [n, 4]: sqrt(-2 ln u1) cos(a) in float64, u1 = ((w0 >> 8) + 1) / 2^24 and u2 = (w1 >> 8) / 2^24
    (both exact in float32), a the angle the sampler's formula hands its cosine: the float32 product of float32(2 pi) and u2.
    (With the angle in float64 instead, a draw whose cosine is near zero would be compared to the rounding of the angle, not to
    the device's arithmetic: |d cos| = |sin a| ulp(a) / 2 is up to 2.4e-7 absolute, whatever the size of the result.)"""
    w = words.astype(np.int64) & 0xFFFFFFFF
    u1 = ((w[:, 0] >> 8) + 1) / 2.0 ** 24
    u2 = ((w[:, 1] >> 8) / 2.0 ** 24).astype(np.float32)
    a = (np.float32(6.28318530717958647692) * u2).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(a)


@pytest.mark.parametrize("word3", [0, 257])
@pytest.mark.parametrize("kind,width,per_atom", [(1, 3, True), (0, 3, False), (2, S, True)],
                         ids=["per-atom", "per-crystal", "species"])
def test_filled_draws_are_the_python_restatement(dev, fused_model, kind, width, per_atom, word3):
    eng = fused_model[0].engine()
    t = 37
    streams = keyed.stream_seeds(SEED, KEYS)
    kw = dict(per_atom_width=width) if per_atom else dict(per_crystal_width=width)
    out, raw = eng.philox_fill_crystals(_seeds(dev, SEED, KEYS), _offsets(dev, COUNTS), t, kind, word3=word3, raw=True, **kw)
    out, raw = out.cpu().numpy(), raw.cpu().numpy()
    rows = sum(COUNTS) if per_atom else len(COUNTS)
    assert out.shape == (rows, width) and raw.shape == (rows, width, 4)
    first = np.concatenate([[0], np.cumsum(COUNTS)])
    want = np.empty((rows, width, 4), dtype=np.int64)
    for b, stream in enumerate(streams):
        n_rows = COUNTS[b] if per_atom else 1
        for a in range(n_rows):
            for c in range(width):
                want[(first[b] if per_atom else b) + a, c] = keyed.raw_words(int(stream), t, kind, a * width + c, word3)
    assert np.array_equal(raw.astype(np.int64) & 0xFFFFFFFF, want)
    if kind == 2:  # uniforms: exact
        u = np.array([[keyed.uniform(int(streams[b]), t, kind, a * width + c, word3) for c in range(width)]
                      for b in range(len(COUNTS)) for a in range(COUNTS[b])])
        assert np.array_equal(out.astype(np.float64), u)
    else:  # normals: the Box-Muller of those words to 4 ulp (float32)
        z = _box_muller(want.reshape(-1, 4)).reshape(rows, width)
        ulp = np.spacing(np.abs(z).astype(np.float32)).astype(np.float64)
        err = np.abs(out.astype(np.float64) - z) / ulp
        print(f"normals, kind {kind}, word3 {word3}: largest error {err.max():.2f} ulp")
        assert (err <= 4).all()


def test_normals_of_one_stream_have_unit_moments(dev, fused_model):
    eng = fused_model[0].engine()
    n = 200000
    z = eng.philox_fill_crystals(_seeds(dev, SEED, [4711]), _offsets(dev, [1]), 3, 14, per_crystal_width=n).double()
    assert z.shape == (1, n)
    assert abs(float(z.mean())) <= 5 / np.sqrt(n)
    assert abs(float(z.var(unbiased=False)) - 1) <= 5 * np.sqrt(2 / n)


# -------------------------------------------------------------------------------------------------------------- independence
def _template(counts, seed=3):
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    rng = np.random.RandomState(seed)
    per = []
    for n in counts:  # (drawn crystal by crystal: a crystal's template does not depend on which others are asked for)
        lengths, angles = rng.uniform(3, 6, 3), np.deg2rad(rng.uniform(75, 105, 3))
        per.append((rng.uniform(0, 1, (n, 3)), rng.randint(1, S - 1, n).astype(np.float64), lengths, angles))
    return per, SampleResult


def _crystals(idx, counts=COUNTS):
    """The template crystals `idx` as a SampleResult."""
    from oracle.geometry import lattice_from_params  # (float64, on the host)
    per, SampleResult = _template(counts)
    na = np.array([counts[i] for i in idx], dtype=np.int64)
    cells = lattice_from_params(torch.tensor(np.array([per[i][2] for i in idx])), torch.tensor(np.array([per[i][3] for i in idx]))).numpy()
    return SampleResult(frac_x=np.concatenate([per[i][0] for i in idx]), atomic_numbers=np.concatenate([per[i][1] for i in idx]),
                        lattice=cells, num_atoms=na, idx_start=np.cumsum(na) - na)


def _cubic_spec():
    from arreau_amd.diffusion import symmetry as sy
    return sy.SymmetrySpec.general_positions(["z,x,y", "-x,-y,z"], 1, "cubic")  # P23: 12 general positions


def _run_case(m, name, idx, use_graph):
    """sample() of the crystals `idx` of the case's three, keyed by KEYS[idx]."""
    from arreau_amd.diffusion.conditioning import SampleCondition
    keys = [KEYS[i] for i in idx]
    counts = [COUNTS[i] for i in idx]
    kw = dict(num_steps=6, seed=SEED, crystal_keys=keys, use_graph=use_graph)
    if name == "plain":
        pass
    elif name == "eta":
        kw.update(eta=0.5)
    elif name == "corrector-resampling":
        kw.update(corrector_steps=1, resample_passes=2, jump_length=2)
    elif name == "multistep":
        kw.update(multistep=True)
    elif name == "symmetry":
        spec = _cubic_spec()
        specs, systems, all_counts = [spec, None, spec], ["cubic", None, "cubic"], [12, 7, 12]
        return m.sample([all_counts[i] for i in idx], len(idx), symmetry=[specs[i] for i in idx],
                        lattice_system=[systems[i] for i in idx], **kw), [all_counts[i] for i in idx]
    elif name == "elements":
        sets = [["Li", "O"], None, [5, 6]]
        kw.update(elements=[sets[i] for i in idx], species_temperature=0.5)
    elif name == "condition":  # a template with one known atom (position and species) in the first and in the last crystal
        tmpl = _crystals(idx)
        known = np.concatenate([np.arange(COUNTS[i]) == (1 if i != 1 else -1) for i in idx])
        cond = SampleCondition.from_sample_result(tmpl, fix_positions=known, fix_species=known)
        return m.sample(condition=cond, **kw), counts
    elif name == "condition-lattice":  # the first and the last crystal's cells known (their lengths forward-noised with kind 4)
        tmpl = _crystals(idx)
        known = np.concatenate([np.arange(COUNTS[i]) == (0 if i == 2 else -1) for i in idx])
        cond = SampleCondition.from_sample_result(tmpl, fix_positions=known, fix_species=False, fix_lattice=np.array([i != 1 for i in idx]))
        return m.sample(condition=cond, **kw), counts
    elif name == "noise_to":
        state = m.noise_to(_crystals(idx), 40, seed=SEED, crystal_keys=keys)
        return m.sample(initial_state=state, **kw), counts
    elif name == "fixed_cell":
        kw.update(fixed_cell=True)
    else:
        raise AssertionError(name)
    return m.sample(counts, len(idx), **kw), counts


def _per_crystal(res, counts):
    first = np.concatenate([[0], np.cumsum(counts)])
    return [(res.frac_x[first[b]:first[b + 1]].tobytes(), res.atomic_numbers[first[b]:first[b + 1]].tobytes(), res.lattice[b].tobytes())
            for b in range(len(counts))]


CASES = ["plain", "eta", "corrector-resampling", "multistep", "symmetry", "elements", "condition", "condition-lattice", "noise_to",
         "fixed_cell"]


@pytest.mark.parametrize("name", CASES)
def test_a_crystal_does_not_depend_on_its_batch(dev, fused_model, name):
    """Keys [11, 4, 29] as one batch, each crystal alone, and as [29, 11]: every crystal's positions, species and cell are bitwise
    the same wherever it ran, eager and under graph replay (the cell stands for the lengths too: a result holds the cell, formed
    on the device from the lengths and the angles).  The host generators are not touched."""
    m, _ = fused_model
    torch.manual_seed(1)
    np.random.seed(1)
    t_state, n_state = torch.random.get_rng_state(), np.random.get_state()
    runs = {}
    for use_graph in (False, True):
        for idx in ([0, 1, 2], [0], [1], [2], [2, 0]):
            res, counts = _run_case(m, name, idx, use_graph)
            assert res.crystal_keys.tolist() == [KEYS[i] for i in idx]
            assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all(), (name, idx)
            runs[(use_graph, tuple(idx))] = dict(zip(idx, _per_crystal(res, counts)))
    want = runs[(False, (0, 1, 2))]
    assert len({want[i][0] for i in (0, 1, 2)}) == 3  # three different crystals
    for (use_graph, idx), got in runs.items():
        for i, crystal in got.items():
            for part, a, b in zip(("frac_x", "species", "lattice"), crystal, want[i]):
                assert a == b, (name, "graph" if use_graph else "eager", idx, i, part)
    assert torch.equal(torch.random.get_rng_state(), t_state)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), n_state))


@pytest.mark.parametrize("option", ["plain", "tied", "corrector-resampling"])
def test_a_crystal_of_the_keyed_loop_does_not_depend_on_its_batch(dev, fused_model, option):
    """The same at the engine, where the lengths are at hand: the keyed loop on a state of three crystals, on each crystal's state
    alone and on crystals [2, 0] -- positions, species, lengths and cell of every crystal bitwise the same."""
    m, _ = fused_model
    eng = m.engine()
    case = Batch(dev, seed=37)
    first = np.concatenate([[0], np.cumsum(COUNTS)])
    steps = [70, 40, 20, 1]
    ties = [1, 2, 0]
    runs = {}
    for use_graph in (False, True):
        for idx in ([0, 1, 2], [0], [1], [2], [2, 0]):
            rows = torch.as_tensor(np.concatenate([np.arange(first[i], first[i + 1]) for i in idx]), device=dev)
            crystals = torch.as_tensor(idx, device=dev)
            full = case.fresh()
            f, ty, le = full[0][rows].contiguous(), full[1][rows].contiguous(), full[2][crystals].contiguous()
            lat = torch.zeros(len(idx), 3, 3, device=dev)
            kw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP, use_graph=use_graph,
                      crystal_seeds=_seeds(dev, SEED, [KEYS[i] for i in idx]))
            if option == "tied":
                kw.update(length_tie=torch.as_tensor([ties[i] for i in idx], dtype=torch.int32, device=dev))
            elif option == "corrector-resampling":
                kw.update(corrector=(1, SNR), resampling=(2, 2, steps))
            counts = [COUNTS[i] for i in idx]
            eng.sample_loop(f, ty, le, case.an[crystals].contiguous(), _offsets(dev, counts), steps[0], len(steps), SEED, None, lat, **kw)
            sub = np.concatenate([[0], np.cumsum(counts)])
            for j, i in enumerate(idx):
                runs[(use_graph, tuple(idx), i)] = (f[sub[j]:sub[j + 1]].clone(), ty[sub[j]:sub[j + 1]].clone(), le[j].clone(), lat[j].clone())
    eng.check_status()
    for (use_graph, idx, i), got in runs.items():
        assert_same_bits(got, runs[(False, (0, 1, 2), i)], (option, use_graph, idx, i))
    assert not torch.equal(runs[(False, (0, 1, 2), 0)][2], runs[(False, (0, 1, 2), 2)][2])
    if option == "tied":
        le = runs[(False, (0, 1, 2), 1)][2]
        assert float(le[0]) == float(le[1]) == float(le[2])


def test_keys_matter(dev, fused_model):
    m, _ = fused_model
    run = lambda seed, keys: m.sample(COUNTS, 3, num_steps=6, seed=seed, crystal_keys=keys)
    a, b, c = run(5, [1, 2, 3]), run(5, [1, 2, 3]), run(5, [4, 2, 6])
    for x, y in zip(_per_crystal(a, COUNTS), _per_crystal(b, COUNTS)):
        assert x == y  # the same (seed, key) twice
    pa, pc = _per_crystal(a, COUNTS), _per_crystal(c, COUNTS)
    assert pa[1] == pc[1] and pa[0][0] != pc[0][0] and pa[2][0] != pc[2][0]  # different keys under one seed
    d, e = run(5, [1, 8, 9]), run(6, [0, 8, 9])
    pd, pe = _per_crystal(d, COUNTS), _per_crystal(e, COUNTS)
    assert pd[0][0] != pe[0][0] and pd[0][2] != pe[0][2]  # (seed 5, key 1) is not (seed 6, key 0)
    assert pd[1][0] != pe[1][0]  # nor is the same key under another seed
    assert pd[0] == pa[0]
    # control: without keys the same comparison tells a crystal in a batch from the crystal alone (the draws follow the batch)
    def unkeyed(counts):
        torch.manual_seed(9)
        np.random.seed(9)
        return m.sample(counts, len(counts), num_steps=6, seed=5)
    assert _per_crystal(unkeyed(COUNTS), COUNTS)[1][0] != _per_crystal(unkeyed(COUNTS[1:2]), COUNTS[1:2])[0][0]


# -------------------------------------------------------------------------------------------------------------- loop against steps
def _keyed_noise(eng, seeds, off, t, w):
    """(z_lattice [B,3], z_frac [N,3], u_types [N,S]) of the step at t with counter word w, from arreau_philox_fill_crystals."""
    return (eng.philox_fill_crystals(seeds, off, t, 0, word3=w, per_crystal_width=3), eng.philox_fill_crystals(seeds, off, t, 1, word3=w, per_atom_width=3),
            eng.philox_fill_crystals(seeds, off, t, 2, word3=w, per_atom_width=S))


@pytest.mark.parametrize("option", ["plain", "corrector-resampling"])
def test_keyed_loop_is_its_steps_fed_the_filled_draws(dev, fused_model, option):
    """Three steps of arreau_sample_loop_keyed against predict_scores + the caller's-noise exports fed arreau_philox_fill_crystals:
    bit for bit (the corrector + resampling case: its events one by one, jumps and corrector moves included)."""
    m, _ = fused_model
    eng = m.engine()
    case = Batch(dev, seed=23)
    B, N = case.B, case.N
    seeds = _seeds(dev, SEED, KEYS)
    steps = [60, 30, 1]
    R, J, M = (2, 2, 1) if option != "plain" else (1, 10, 0)
    ctl = (None, 1.0)
    f, ty, le, lat = case.fresh()
    for ev in rs.plan(steps, 0, R, J):
        if ev.kind == "jump":
            eng.resample_jump(f, ty, le, case.an, full_i32(B, ev.s, dev), full_i32(B, ev.t, dev), case.off,
                              eng.philox_fill_crystals(seeds, case.off, ev.t, 6, word3=ev.r, per_atom_width=3),
                              eng.philox_fill_crystals(seeds, case.off, ev.t, 7, word3=ev.r, per_crystal_width=3),
                              eng.philox_fill_crystals(seeds, case.off, ev.t, 8, word3=ev.r, per_atom_width=S), lat)
            continue
        t, w = ev.t, 256 * ev.r
        t_c = full_i32(B, t, dev)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        for j in range(M):
            eng.corrector_step(f, t_c, case.off, eps, eng.philox_fill_crystals(seeds, case.off, t, 5, word3=w + j, per_atom_width=3), SNR)
            eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        z_l, z_f, u_t = _keyed_noise(eng, seeds, case.off, t, w)
        eng.reverse_step_species(f, ty, le, case.an, t_c, full_i32(B, ev.s, dev), case.off, eps, logits, len0, z_l, z_f, u_t, lat, ctl,
                                 lattice_clipmax=CLIP)
    kw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP, crystal_seeds=seeds)
    if option != "plain":
        kw.update(corrector=(M, SNR), resampling=(R, J, steps))
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop(*got[:3], case.an, case.off, steps[0], len(steps), SEED, None, got[3], use_graph=use_graph, **kw)
        assert_same_bits(got, (f, ty, le, lat), (option, use_graph))
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- segments
def test_keyed_run_in_segments_is_the_run_in_one_call(dev, fused_model, tmp_path):
    from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting
    m, _ = fused_model
    kw = dict(timesteps=[99, 70, 40, 20, 10, 1], seed=SEED, crystal_keys=KEYS)
    whole = m.sample(COUNTS, 3, **kw)
    framed = m.sample(COUNTS, 3, visualization_setting=VisualizationSetting.ALL_DETAILED, vis_name=str(tmp_path / "f"), **kw)
    assert _per_crystal(framed, COUNTS) == _per_crystal(whole, COUNTS)
    # cut by max_steps: the state after three steps, handed on as an initial state, ends where the whole run ends
    eng = m.engine()
    case = Batch(dev, seed=29)
    seeds = _seeds(dev, SEED, KEYS)
    steps = [80, 60, 45, 30, 10, 1]
    lkw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP, crystal_seeds=seeds)
    one = case.fresh()
    eng.sample_loop(*one[:3], case.an, case.off, steps[0], len(steps), SEED, None, one[3], **lkw)
    cut = case.fresh()
    for lo, hi in ((0, 1), (1, 4), (4, 6)):
        eng.sample_loop(*cut[:3], case.an, case.off, steps[lo], hi - lo, SEED, None, cut[3], use_graph=hi - lo >= 3, **lkw)
    assert_same_bits(cut, one, "segments")
    a = m.sample(COUNTS, 3, max_steps=3, **kw)
    b = m.sample(COUNTS, 3, max_steps=3, **kw)
    assert _per_crystal(a, COUNTS) == _per_crystal(b, COUNTS) and _per_crystal(a, COUNTS) != _per_crystal(whole, COUNTS)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- the default path
def test_default_path_is_untouched(dev, fused_model, monkeypatch):
    """crystal_keys=None dispatches to the export it used before; a NULL table to arreau_sample_loop_keyed is
    arreau_sample_loop_species bit for bit."""
    import ctypes

    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    lib = _hip.lib()
    called = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("arreau_sample_loop"):
                called.append(name)
            return fn
    monkeypatch.setattr(_hip, "lib", lambda: Spy())
    m.sample(COUNTS, 3, max_steps=3, seed=SEED)
    assert set(called) == {"arreau_sample_loop"}
    called.clear()
    m.sample(COUNTS, 3, max_steps=3, seed=SEED, species_temperature=0.5)
    assert set(called) == {"arreau_sample_loop_species"}
    called.clear()
    m.sample(COUNTS, 3, max_steps=3, seed=SEED, crystal_keys=KEYS)
    assert set(called) == {"arreau_sample_loop_keyed"}
    monkeypatch.undo()
    # the NULL table, called directly
    case = Batch(dev, seed=31)
    steps = [50, 30, 20, 1]
    nxt = respacing.next_table(T, steps).to(dev)
    want = case.fresh()
    eng.sample_loop_species(*want[:3], case.an, case.off, steps[0], len(steps), SEED, None, want[3], (None, 0.5), next_table=nxt,
                            lattice_clipmax=CLIP)
    got = case.fresh()
    ws = eng.workspace(case.N, case.B)
    sched = _hip.SampleScheduleC(_hip.ptr(nxt).value, CLIP)
    ctl = _hip.SpeciesControlC(None, 0.5)
    _hip.check(lib.arreau_sample_loop_keyed(
        eng._handle, _hip.ptr(got[0]), _hip.ptr(got[1]), _hip.ptr(got[2]), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N, steps[0],
        len(steps), SEED, None, None, _hip.ptr(got[3]), _hip.ptr(ws), ws.numel(), 0, None, ctypes.byref(sched), None, None, None, None, None,
        None, ctypes.byref(ctl), None, _hip.stream_ptr(dev)), "arreau_sample_loop_keyed")
    assert_same_bits(got, want, "NULL table")
    keyed_run = case.fresh()
    eng.sample_loop(*keyed_run[:3], case.an, case.off, steps[0], len(steps), SEED, None, keyed_run[3], species=(None, 0.5), next_table=nxt,
                    lattice_clipmax=CLIP, crystal_seeds=_seeds(dev, SEED, KEYS))
    assert not torch.equal(keyed_run[0], want[0])  # the table is read
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- two ranks
def test_generate_keyed_writes_the_same_file_at_one_and_two_ranks(dev, tmp_path):
    """python -m arreau_amd.generate --keyed at world size 1 and 2 (gloo, the ranks taking turns on this box's one GPU): the two
    files agree array for array."""
    import socket
    import subprocess
    import sys

    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=12, seed=3, num_timesteps=30))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(ARREAU_GENERATE_BACKEND="gloo", ARREAU_GENERATE_ONE_DEVICE="1", PYTHONPATH=root, ARREAU_GENERATE_GPU_LOCK=str(tmp_path / "gpu.lock"))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    common = ["-m", "arreau_amd.generate", "--model_path", ckpt, "--keyed", "--seed", "3", "--num_crystals", "6", "--num_atoms", "4",
              "--num_steps", "5"]
    out1, out2 = str(tmp_path / "one" / "crystals.npz"), str(tmp_path / "two" / "crystals.npz")
    subprocess.run([sys.executable] + common + ["--out", out1], check=True, env=env, cwd=root, timeout=600)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", str(port)] + common + ["--batch", "2", "--out", out2], check=True, env=env, cwd=root, timeout=600)
    with np.load(out1) as one, np.load(out2) as two:
        assert one.files == two.files and "crystal_keys" in one.files
        assert one["crystal_keys"].tolist() == list(range(6))
        for k in one.files:
            assert one[k].dtype == two[k].dtype and one[k].tobytes() == two[k].tobytes(), k
        assert np.isfinite(one["frac_x"]).all() and len({one["frac_x"][4 * b:4 * b + 4].tobytes() for b in range(6)}) == 6


def test_generate_keyed_start_from_writes_the_same_file_at_one_and_two_ranks(dev, tmp_path):
    """generate --keyed --start_from FILE --start_t K at world size 1 and 2 with different --batch: the crystals of the file, keyed
    by their index, are noised and denoised to the same bits wherever they ran; every one moved away from where it started."""
    import socket
    import subprocess
    import sys

    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import save_sample_results_to_hdf5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=12, seed=3, num_timesteps=30))
    counts = [4, 2, 5, 3, 4]
    start = save_sample_results_to_hdf5(_crystals(list(range(5)), counts), str(tmp_path / "start.npz"))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(ARREAU_GENERATE_BACKEND="gloo", ARREAU_GENERATE_ONE_DEVICE="1", PYTHONPATH=root, ARREAU_GENERATE_GPU_LOCK=str(tmp_path / "gpu.lock"))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    common = ["-m", "arreau_amd.generate", "--model_path", ckpt, "--keyed", "--seed", "3", "--start_from", start, "--start_t", "12",
              "--num_steps", "4"]
    out1, out2 = str(tmp_path / "one" / "crystals.npz"), str(tmp_path / "two" / "crystals.npz")
    subprocess.run([sys.executable] + common + ["--out", out1], check=True, env=env, cwd=root, timeout=600)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", str(port)] + common + ["--batch", "2", "--out", out2], check=True, env=env, cwd=root, timeout=600)
    with np.load(out1) as one, np.load(out2) as two, np.load(start) as given:
        assert one.files == two.files and one["crystal_keys"].tolist() == list(range(5)) and one["num_atoms"].tolist() == counts
        for k in one.files:
            assert one[k].dtype == two[k].dtype and one[k].tobytes() == two[k].tobytes(), k
        assert np.isfinite(one["frac_x"]).all() and not np.array_equal(one["frac_x"], given["frac_x"])
