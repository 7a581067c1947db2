"""The sampler's Python front end without a GPU: the resolved plan of a sample() call (diffusion/sample_plan.py), the engine's
export table and step ladder driven through a recording library, and the host-noise driver on a recording engine."""
import ctypes

import numpy as np
import pytest
import torch

from arreau_amd import _hip, engine as engine_mod
from arreau_amd.diffusion import contact_guidance as cg, diffusion_loss as dl_mod, multistep as ms, sample_plan
from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting as VS
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable

ZT = AtomicNumberTable([1, 6, 8, 14, 2001])
T, N, B, S = 100, 5, 2, 5
BATCH = dict(num_atoms_per_sample=[2, 3], num_samples_in_batch=2)


# ---------------------------------------------------------------------------------------------------------------- the plan
def test_resolve_takes_no_model_and_reads_no_generator():
    np.random.seed(5)
    torch.manual_seed(5)
    before = np.random.get_state()[1].copy(), torch.random.get_rng_state().clone()
    plan = sample_plan.resolve(T, ZT, elements=["H", "C"], crystal_keys=[3, 9], seed=1, screen=True, bond_order=True, **BATCH)
    assert (plan.B, plan.N, plan.S, plan.noise) == (2, 5, 5, "philox") and plan.num_atoms.tolist() == [2, 3]
    assert plan.instruments["screen"] is not None and plan.instruments["unique"] is None and plan.crystal_keys.tolist() == [3, 9]
    assert len(plan.allow_rows) == 2 and plan.crystal_of.tolist() == [0, 0, 1, 1, 1]
    with pytest.raises(ValueError, match="one class index per atom"):  # (the parent drew the whole initial state first)
        sample_plan.resolve(T, ZT, constant_atoms=torch.tensor([0, 1, 2]), **BATCH)
    with pytest.raises(ValueError, match="need noise='philox'"):
        sample_plan.resolve(T, ZT, fixed_cell=True, noise="reference", **BATCH)
    assert np.array_equal(np.random.get_state()[1], before[0]) and torch.equal(torch.random.get_rng_state(), before[1])


def _steps(events):
    return [(e.kind, e.t, e.s, e.r) for e in events]


def test_plan_of_the_full_schedule_cut_by_max_steps_with_frames():
    plan = sample_plan.resolve(T, ZT, visualization_setting=VS.ALL, vis_name="f", max_steps=25, **BATCH)
    assert plan.schedule is None and plan.successor is None and (plan.top, plan.t_first) == (99, 99)
    assert plan.steps == list(range(99, 74, -1))
    assert plan.stops == [9, 19] and [plan.steps[j] for j in plan.stops] == [90, 80]  # never the first step, every 10th timestep
    assert _steps(plan.events) == [("step", t, t - 1, 0) for t in range(99, 74, -1)]
    assert plan.use_graph is False and plan.corrector is None and plan.resampling is None


def test_plan_of_an_explicit_schedule_with_detailed_frames():
    ts = [99, 60, 50, 45, 1]
    plan = sample_plan.resolve(T, ZT, timesteps=ts, visualization_setting=VS.ALL_DETAILED, vis_name="f", noise="reference", **BATCH)
    assert plan.steps == ts and plan.schedule == ts and plan.t_first == 99
    assert plan.successor == {99: 60, 60: 50, 50: 45, 45: 1, 1: 0}
    assert plan.stops == [1, 2, 3, 4]
    assert _steps(plan.events) == [("step", 99, 60, 0), ("step", 60, 50, 0), ("step", 50, 45, 0), ("step", 45, 1, 0), ("step", 1, 0, 0)]


def test_plan_of_resampling_on_six_scheduled_steps():
    ts = [90, 70, 50, 30, 10, 1]
    plan = sample_plan.resolve(T, ZT, timesteps=ts, resample_passes=2, jump_length=2, corrector_steps=1, **BATCH)
    assert plan.steps == ts and plan.stops == [] and plan.resampling == (2, 2, ts) and plan.corrector == (1, sample_plan.pc.DEFAULT_SNR)
    block = lambda a, b, c, r: [("step", a, b, r), ("step", b, c, r)]
    assert _steps(plan.events) == (block(90, 70, 50, 0) + [("jump", 90, 50, 1)] + block(90, 70, 50, 1)
                                   + block(50, 30, 10, 0) + [("jump", 50, 10, 1)] + block(50, 30, 10, 1)
                                   + block(10, 1, 0, 0) + [("jump", 10, 0, 1)] + block(10, 1, 0, 1))
    assert plan.use_graph is False
    assert sample_plan.resolve(T, ZT, resample_passes=2, jump_length=2, **BATCH).use_graph is False       # 99 x 2 < 200
    assert sample_plan.resolve(T, ZT, resample_passes=3, jump_length=2, **BATCH).use_graph is True        # 99 x 3 >= 200


# --------------------------------------------------------------------------------------------- the engine's export table
class RecordingLib:
    """Stands in for the shared library: records (export, arguments) and returns 0."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == "arreau_workspace_bytes":
            return lambda *a: 64

        def export(*args):
            self.calls.append((name, args))
            return 0
        return export


@pytest.fixture
def lib(monkeypatch):
    rec = RecordingLib()
    monkeypatch.setattr(_hip, "lib", lambda: rec)
    monkeypatch.setattr(_hip, "stream_ptr", lambda device=None: "stream")
    return rec


def _engine():
    eng = engine_mod.HipEngine.__new__(engine_mod.HipEngine)  # no GPU: the struct builders and the dispatch use only .device
    eng.device, eng.cfg, eng._handle, eng._ws, eng._ws_cap, eng.S = torch.device("cpu"), _hip.Config(num_timesteps=T), "H", None, (0, 0), S
    return eng


def _tensors():
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
    i = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    t = dict(frac=f(N, 3), types=i(N), lengths=f(B, 3), angles=f(B, 3), off=i(B + 1), lattice=f(B, 3, 3), t=i(B), s=i(B), eps=f(N, 3),
             logits=f(N, S), len0=f(B, 3), zl=f(B, 3), zf=f(N, 3), u=f(N, S), tie=i(B), nxt=i(T + 1), allow=i(B, 4),
             seeds=torch.zeros(B, dtype=torch.int64))
    t["sym"] = dict({n: i(N) for n in ("leader", "op", "orbit")}, orbit_ptr=i(3), orbit_atoms=i(N), stab_ptr=i(3), stab_ops=i(4),
                    rot=f(2, 9), rot_inv=f(2, 9), trans=f(2, 3))
    t["hist"] = {"hist_eps": f(N, 3), "hist_x0": f(B, 3), "hist_t_atom": i(N), "hist_t_len": i(B)}
    assert set(t["hist"]) == set(ms.HISTORY_KEYS)
    return t


def _null(arg):
    return arg is None or (isinstance(arg, ctypes.c_void_p) and not arg.value)


# (export, the options of the call, the NULL pattern of what follows the 17 common arguments: 1 = given, 0 = NULL)
LOOP_CASES = [
    ("arreau_sample_loop", {}, ""),
    ("arreau_sample_loop_resampled", {"corrector": (2, 0.16)}, "0010"),
    ("arreau_sample_loop_resampled", {"next_table": "nxt", "resampling": (2, 3, [90, 50, 1])}, "0101"),
    ("arreau_sample_loop_tied", {"length_tie": "tie"}, "0000" "1"),
    ("arreau_sample_loop_eta", {"eta": 0.5}, "0000" "01"),
    ("arreau_sample_loop_sym", {"symmetry": "sym"}, "0000" "01"),
    ("arreau_sample_loop_multistep", {"multistep": "hist", "length_tie": "tie"}, "0000" "11"),
    ("arreau_sample_loop_species", {"species": (None, 0.5), "eta": 0.0}, "0000" "00101"),
    ("arreau_sample_loop_species", {"species": ("allow", 1.0), "multistep": "hist", "eta": 0.0}, "0000" "00011"),  # multistep: no eta
    ("arreau_sample_loop_keyed", {"crystal_seeds": "seeds", "symmetry": "sym"}, "0000" "01001" "1"),
    ("arreau_sample_loop_guided", {"guidance": cg.ContactGuidance()}, "0000" "00001" "01"),
    ("arreau_sample_loop_guided", {"guidance": cg.ContactGuidance(), "crystal_seeds": "seeds", "length_tie": "tie"}, "0000" "10001" "11"),
]


@pytest.mark.parametrize("export,options,pattern", LOOP_CASES, ids=[f"{c[0][7:]}-{i}" for i, c in enumerate(LOOP_CASES)])
def test_sample_loop_selects_its_export_by_table(lib, export, options, pattern):
    """One option set per row of engine._LOOP_EXPORTS (the nine exports sample_loop can reach) and the precedence between rows."""
    t = _tensors()
    named = lambda v: t[v] if isinstance(v, str) else tuple(named(x) for x in v) if isinstance(v, tuple) else v
    _engine().sample_loop(t["frac"], t["types"], t["lengths"], t["angles"], t["off"], 90, 3, 7, None, t["lattice"],
                          **{k: named(v) for k, v in options.items()})
    (name, args), = lib.calls
    assert name == export
    assert args[0] == "H" and args[6:10] == (B, N, 90, 3) and args[-1] == "stream"
    assert "".join("0" if _null(a) else "1" for a in args[17:-1]) == pattern
    if export == "arreau_sample_loop_eta":
        assert isinstance(args[-2], ctypes.c_float) and args[-2].value == 0.5  # by value; the species family takes a pointer
    if "eta" in options and export == "arreau_sample_loop_species" and "multistep" not in options:
        assert args[17 + 6]._obj.value == 0.0


def test_the_export_table_reads_in_the_stated_precedence():
    assert [row[0][len("arreau_sample_loop"):] for row in engine_mod._LOOP_EXPORTS] == \
        ["_guided", "_keyed", "_species", "_multistep", "_sym", "_eta", "_tied", "_resampled", ""]


STEP_CASES = [  # (species, multistep, eta, tied, scheduled) -> export; s_crystal is written for every export but the plain one
    ((1, 1, 1, 1, 1), "arreau_reverse_step_species"), ((1, 0, 0, 0, 0), "arreau_reverse_step_species"),
    ((0, 1, 1, 1, 1), "arreau_reverse_step_multistep"), ((0, 0, 1, 1, 0), "arreau_reverse_step_eta"),
    ((0, 0, 0, 1, 0), "arreau_reverse_step_tied"), ((0, 0, 0, 0, 1), "arreau_reverse_step_to"), ((0, 0, 0, 0, 0), "arreau_reverse_step"),
]


@pytest.mark.parametrize("given,export", STEP_CASES)
def test_predictor_step_picks_the_step_export_by_its_ladder(lib, given, export):
    t = _tensors()
    species, history, eta, tie, scheduled = given
    t["s"].fill_(-1)
    _engine().predictor_step(t["frac"], t["types"], t["lengths"], t["angles"], t["t"], t["s"], t["off"], t["eps"], t["logits"], t["len0"],
                             t["zl"], t["zf"], t["u"], t["lattice"], 42, scheduled=bool(scheduled), length_tie=t["tie"] if tie else None,
                             eta=0.25 if eta else None, multistep=t["hist"] if history else None,
                             species=(t["allow"], 0.5) if species else None, lattice_clipmax=0.98)
    (name, args), = lib.calls
    assert name == export
    assert t["s"].tolist() == ([-1, -1] if export == "arreau_reverse_step" else [42, 42])
    if export != "arreau_reverse_step":
        assert args[6].value == t["s"].data_ptr() and args[5].value == t["t"].data_ptr()
    if export == "arreau_reverse_step_multistep":
        assert _null(args[13]) and _null(args[14]) and args[15].value == t["u"].data_ptr()  # no position or length draw is read
    if given == (1, 1, 1, 1, 1):
        assert _null(args[-4])  # eta is not handed on beside a history: the multistep step is the eta = 0 step


def test_tensor_contract_messages():
    dev = torch.device("cpu")
    ok = torch.zeros(3, dtype=torch.int32)
    engine_mod._require("", "length_tie", ok, (3,), torch.int32, dev)
    with pytest.raises(ValueError, match=r"^length_tie must be a contiguous int32 tensor of shape \(2,\) on cpu$"):
        engine_mod._require("", "length_tie", ok, (2,), torch.int32, dev)
    with pytest.raises(ValueError, match=r"^condition: x0 must be a contiguous torch.float32 tensor of shape \(3, 3\) on cpu$"):
        engine_mod._require("condition", "x0", torch.zeros(6, 3)[::2], (3, 3), torch.float32, dev)
    with pytest.raises(ValueError, match=r"^symmetry tables: rot must be a non-empty contiguous torch.float32 tensor on cpu$"):
        engine_mod._require("symmetry tables", "rot", torch.zeros(0, 9), None, torch.float32, dev)
    with pytest.raises(ValueError, match="^guidance info: energy must be"):
        _engine()._guidance_struct((cg.ContactGuidance(), {"energy": None, "contacts": ok[:2], "flags": ok[:2]}), 2)


# ------------------------------------------------------------------------------------------------- the host-noise driver
class RecordingEngine:
    """Records the engine calls of a run; the network predicts zeros and a step moves the species, so a held species shows."""
    def __init__(self):
        self.calls, self.device = [], torch.device("cpu")

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name, tuple(a.clone() if torch.is_tensor(a) else a for a in args), kw))  # (the buffers are reused)
            if name == "predict_scores":
                return torch.zeros(N, 3), torch.zeros(N, S), torch.zeros(B, 3)
            if name == "predictor_step":
                args[1].add_(1)
        return call


@pytest.mark.parametrize("noise", ["reference", "device"])
def test_host_noise_driver_issues_the_events_in_order(noise, monkeypatch):
    draws = []
    real_randn, real_rand = torch.randn, torch.rand
    monkeypatch.setattr(torch, "randn", lambda shape, **kw: (draws.append(("normal", tuple(shape))), real_randn(shape, dtype=kw.get("dtype")))[1])
    monkeypatch.setattr(torch, "rand", lambda shape, **kw: (draws.append(("uniform", tuple(shape))), real_rand(shape, dtype=kw.get("dtype")))[1])
    plan = sample_plan.resolve(T, ZT, noise=noise, timesteps=[90, 50, 1], corrector_steps=2, resample_passes=2, jump_length=2,
                               contact_guidance=True, eta=0.5, **BATCH)
    const = torch.tensor([4, 3, 2, 1, 0], dtype=torch.int32)
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
    buf = dl_mod._RunBuffers(frac_d=f(N, 3), types_d=const.clone(), len_d=f(B, 3) + 4, ang_d=f(B, 3) + 1.5, off_d=torch.tensor([0, 2, 5], dtype=torch.int32),
                             lattice_d=f(B, 3, 3), clipmax=0.99, const_d=const, guide=(plan.guidance, {}))
    monkeypatch.setattr(dl_mod, "lattice_from_params", lambda lengths, angles: f(B, 3, 3))  # (a launch of its own: needs the GPU)
    eng = RecordingEngine()
    frames = []
    dl_mod._host_noise_driver(eng, plan, buf, None, False, frames.append)
    names = [c[0] for c in eng.calls]
    evaluation = ["predict_scores", "contact_guidance_step"]
    step = evaluation + ["corrector_step"] + evaluation + ["corrector_step"] + evaluation + ["predictor_step"]
    assert names == step * 2 + ["resample_jump"] + step * 2 + step + ["resample_jump"] + step
    # the draws: per step one normal [N,3] per corrector move, then lengths, positions, species; per jump positions, lengths, species
    step_draws = [("normal", (N, 3))] * 2 + [("normal", (B, 3)), ("normal", (N, 3)), ("uniform", (N, S))]
    jump_draws = [("normal", (N, 3)), ("normal", (B, 3)), ("uniform", (N, S))]
    assert draws == step_draws * 2 + jump_draws + step_draws * 3 + jump_draws + step_draws
    steps = [c for c in eng.calls if c[0] == "predictor_step"]
    assert [(int(c[1][4][0]), c[1][14]) for c in steps] == [(90, 50), (50, 1), (90, 50), (50, 1), (1, 0), (1, 0)]
    assert all(c[2] == dict(scheduled=True, length_tie=None, eta=0.5, multistep=None, species=None, lattice_clipmax=0.99) for c in steps)
    jumps = [c for c in eng.calls if c[0] == "resample_jump"]
    assert [(c[1][4].tolist(), c[1][5].tolist()) for c in jumps] == [([1, 1], [90, 90]), ([0, 0], [1, 1])]  # (s, t): one buffer each
    assert torch.equal(buf.types_d, const) and frames == []  # held species are restored after every step
