"""The resolved plan of a DiffusionLoss.sample call: every keyword checked, cross-checked and turned into what the run needs --
batch layout, schedule, option tuples, frame stops, events -- before an engine, a generator or a directory is touched.  `resolve`
is what "rejected before any work" means, for DiffusionLoss.sample and for PONITA_DIFFUSION.sample alike.  A new sampling option
is one field of SamplePlan and one rule in one of the helpers below.  Host side only: numpy and torch on the CPU, never the
engine."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import contact_guidance as guidance_mod
from . import corrector as pc
from . import ddim
from . import instruments
from . import inversion
from . import keyed as keyed_mod
from . import lattice_systems
from . import multistep as multistep_mod
from . import resampling as rs
from . import respacing
from . import species as species_mod
from . import symmetry as sym_mod
from . import xrd_guidance as xrd_guidance_mod
from .inference.visualize_crystal import VisualizationSetting

NOISE_MODES = ("philox", "device", "reference")


@dataclass(frozen=True)
class SamplePlan:
    instruments: dict            # sample() keyword -> resolved parameters (None: not asked for), the shared-launch rules applied
    guidance: object             # the resolved ContactGuidance or None
    xrd_guidance: object         # the XrdGuidance or None: scattering "Z" or "unit", one target for all crystals or one each
    noise: str
    visualization_setting: object
    num_atoms_per_sample: object  # as draw_initial_state takes it: after the state, the specs or the condition defined the batch
    num_atoms: torch.Tensor      # int64 [B]
    B: int
    N: int
    S: Optional[int]             # len(z_table)
    specs: Optional[list]        # the symmetry specs, one (or None) per crystal; None: no crystal is constrained
    lattice_system: object       # after the specs decided theirs
    schedule: Optional[list]     # None: every timestep
    top: int                     # the level the loop enters at
    steps: list                  # the timesteps this run visits, in order, cut to max_steps
    t_first: int
    successor: Optional[dict]    # scheduled timestep -> the next one (0 after the last); None without a schedule
    corrector: Optional[tuple]   # (steps, snr) or None
    resampling: Optional[tuple]  # (passes, jump_length, schedule) or None
    eta: Optional[float]
    multistep: bool
    species_temperature: float
    allow_rows: Optional[np.ndarray]  # the admission rows of `elements` (None: no set is given) ...
    crystal_of: Optional[np.ndarray]  # ... and with them the crystal of every atom
    crystal_keys: Optional[np.ndarray]
    fixed_cell: bool
    use_graph: bool              # (None resolved: on for at least 200 steps, which amortise capture and instantiation)
    stops: list                  # Philox driver: the indices into `steps` after which the loop is cut for a frame
    events: list                 # host-noise driver: resampling.plan of the visited steps


def frame_after(setting, timestep):
    """Is the state after the step at `timestep` a frame?  (The reference's schedule, diffusion_loss.py:351-370: every 10th for
    ALL, every one for ALL_DETAILED; the drivers leave out the run's first step.)"""
    return (setting == VisualizationSetting.ALL and timestep % 10 == 0) or setting == VisualizationSetting.ALL_DETAILED


def atom_counts(num_atoms_per_sample, B):
    """The atom count of every crystal, int64 [B].  Extension over the reference (uniform n only, diffusion_loss.py:308): a
    sequence gives each crystal of the batch its own atom count (the HIP path works on CSR offsets, so ragged batches cost
    nothing extra)."""
    if isinstance(num_atoms_per_sample, (int, np.integer)):
        return torch.full((B,), int(num_atoms_per_sample))
    num_atoms = torch.as_tensor([int(v) for v in num_atoms_per_sample], dtype=torch.long)
    if num_atoms.numel() != B or int(num_atoms.min()) < 1:
        raise ValueError("num_atoms_per_sample must be an int or hold one positive count per crystal of the batch")
    return num_atoms


def _resolve_instruments(asked):
    """{keyword: resolved parameters or None} of the instrument keywords, then the three rules of the shared launches."""
    out = {e.keyword: e.module.resolve(asked[e.keyword]) for e in instruments.COMPLETE}
    instruments.bond_order.check_shared(out["bond_order"], out["coordination"])
    instruments.symmetrize.check_shared_search(out["symmetrize"], out["find_symmetry"])
    instruments.conventional_cell.check_shared(out["conventional_cell"], out["reduce_cell"], out["find_symmetry"], out["symmetrize"])
    return out


def _resolve_schedule(T, initial_state, z_table, condition, symmetry, lattice_system, num_atoms_per_sample, num_samples_in_batch,
                      num_steps, timesteps):
    """(schedule or None, top, atom counts, batch size): a given state is validated, defines the batch and the level the loop
    enters at."""
    if initial_state is None:
        return respacing.resolve_schedule(T, num_steps=num_steps, timesteps=timesteps), T - 1, num_atoms_per_sample, num_samples_in_batch
    inversion.check_initial_state(initial_state, T, condition=condition, symmetry=symmetry, lattice_system=lattice_system,
                                  num_atoms_per_sample=num_atoms_per_sample, num_samples_in_batch=num_samples_in_batch,
                                  num_atomic_states=len(z_table) if z_table is not None else None)
    counts = [int(v) for v in np.asarray(initial_state.num_atoms).reshape(-1)]
    schedule = inversion.schedule_from(T, initial_state.t, num_steps=num_steps, timesteps=timesteps)
    return schedule, int(initial_state.t), counts, len(counts)


def _resolve_symmetry(symmetry, num_atoms_per_sample, num_samples_in_batch, lattice_system, constant_atoms, unsupported, eta):
    """(specs or None, atom counts, batch size, lattice systems): the specs decide the atom counts and lattice systems.
    `unsupported`: (name, given) of the options the symmetric loop does not take."""
    if symmetry is not None and not isinstance(symmetry, sym_mod.SymmetrySpec) and num_samples_in_batch is None:
        try:
            num_samples_in_batch = len(symmetry)
        except TypeError:
            pass
    specs = sym_mod.resolve(symmetry, num_samples_in_batch)
    if specs is None:
        return None, num_atoms_per_sample, num_samples_in_batch, lattice_system
    unsupported = [name for name, on in unsupported if on]
    if unsupported:
        raise ValueError("symmetry= is not supported with " + ", ".join(unsupported) + " yet (a follow-up); it runs in the "
                         "Philox loop without a condition, correctors or resampling")
    if eta is not None:
        raise ValueError("symmetry= is not supported with eta= (the symmetric step has no DDIM-style form)")
    num_atoms_per_sample, lattice_system = sym_mod.batch_layout(specs, num_atoms_per_sample, lattice_system)
    if constant_atoms is not None:
        ca = np.asarray(torch.as_tensor(constant_atoms).reshape(-1))
        if ca.size == sum(num_atoms_per_sample):
            first = np.concatenate([[0], np.cumsum(num_atoms_per_sample)])
            for b, s_b in enumerate(specs):
                if s_b is not None:
                    s_b.check_species(ca[first[b]:first[b + 1]], f"constant species of crystal {b}")
    return specs, num_atoms_per_sample, len(specs), lattice_system


def _resolve_species(elements, z_table, num_atoms, condition, constant_atoms):
    """(admission rows, crystal of every atom), or (None, None) without `elements`; the held species that need no drawn state --
    a condition's known ones, a constant_atoms tensor -- are checked against their crystal's set."""
    if elements is None:
        return None, None
    B = int(num_atoms.numel())
    allow_rows = species_mod.resolve_elements(elements, z_table, B)
    species_mod.check_rows(allow_rows)
    crystal_of = np.repeat(np.arange(B), num_atoms.numpy())
    if condition is not None and condition.species_known().any():
        known = condition.species_known()
        lut = {int(z): c for c, z in enumerate(z_table.zs)}
        cls = np.array([lut.get(int(z), -1) if k else 0 for z, k in zip(np.asarray(condition.atomic_numbers), known)])
        species_mod.check_held(allow_rows, crystal_of, cls, known, "condition")
    if constant_atoms is not None and constant_atoms is not True and constant_atoms is not False:
        held = np.asarray(torch.as_tensor(constant_atoms).reshape(-1))
        if held.size == crystal_of.size:  # (a wrong size is rejected where the species are read)
            species_mod.check_held(allow_rows, crystal_of, held, np.ones(held.size, bool), "constant_atoms")
    return allow_rows, crystal_of


def _visited(schedule, top, max_steps):
    """(steps, t_first, successor) of a run: every timestep top .. 1 or the schedule's, cut to max_steps."""
    steps = list(range(top, 0, -1)) if schedule is None else schedule
    steps = steps if max_steps is None else steps[:max(0, int(max_steps))]
    successor = None if schedule is None else dict(zip(schedule, schedule[1:] + [0]))
    return steps, top if schedule is None else schedule[0], successor


def check_options(*, vis_name="", visualization_setting=VisualizationSetting.NONE, noise="philox", use_graph=None, seed=None,
                  fixed_cell=False, condition=None, corrector_steps=0, corrector_snr=pc.DEFAULT_SNR, resample_passes=1, jump_length=10,
                  symmetry=None, eta=None, multistep=False, species_temperature=1.0, crystal_keys=None, contact_guidance=None,
                  xrd_guidance=None, **others):
    """The rules that need neither the diffusion nor the batch: every option value on its own and the combinations that are
    rejected whatever the batch.  `resolve` starts with them; PONITA_DIFFUSION.sample runs them before it reads anything of
    itself.  Returns (the fields of SamplePlan these rules decide, passes, jump length); `others` holds the instrument keywords
    and whatever of sample()'s keywords has no rule here."""
    guidance = guidance_mod.resolve(contact_guidance)
    xrd_guidance = xrd_guidance_mod.resolve(xrd_guidance)
    xrd_guidance_mod.check_sampling(xrd_guidance)
    resolved = _resolve_instruments({k: others.get(k) for k in instruments.COMPLETE_KEYWORDS})
    if crystal_keys is not None:  # (the count: resolve)
        crystal_keys = keyed_mod.validate_keys(crystal_keys, None, seed, noise if noise in NOISE_MODES else "philox")
    if visualization_setting != VisualizationSetting.NONE and not vis_name:
        raise ValueError("visualization_setting other than NONE needs vis_name (prefix of the frame files)")
    if noise not in NOISE_MODES:
        raise ValueError("noise must be 'philox', 'device' or 'reference'")
    corrector_steps, corrector_snr = pc.check_corrector(corrector_steps, corrector_snr)
    resample_passes, jump_length = rs.check_resampling(resample_passes, jump_length)
    eta = ddim.check_eta(eta) if eta is not None else None
    multistep = multistep_mod.check_multistep(multistep, eta=eta, condition=condition, corrector_steps=corrector_steps,
                                              resample_passes=resample_passes, symmetry=symmetry)
    species_temperature = species_mod.validate_temperature(species_temperature)
    if resample_passes > 1 and visualization_setting in (VisualizationSetting.ALL, VisualizationSetting.ALL_DETAILED):
        raise ValueError("resampling (resample_passes > 1) takes visualization_setting NONE or LAST: a frame inside a block "
                         "would be overwritten by the block's next pass")
    if (use_graph or fixed_cell) and noise != "philox":
        raise ValueError("graph replay and fixed-cell sampling need noise='philox' (the in-kernel generator)")
    return dict(instruments=resolved, guidance=guidance, xrd_guidance=xrd_guidance, noise=noise, visualization_setting=visualization_setting,
                corrector=(corrector_steps, corrector_snr) if corrector_steps > 0 else None, eta=eta, multistep=multistep,
                species_temperature=species_temperature, crystal_keys=crystal_keys, fixed_cell=bool(fixed_cell)), resample_passes, jump_length


def resolve(T, z_table, *, num_atoms_per_sample=None, num_samples_in_batch=None, constant_atoms=None, max_steps=None,
            num_steps=None, timesteps=None, lattice_system=None, initial_state=None, elements=None, noise="philox", condition=None,
            symmetry=None, seed=None, fixed_cell=False, use_graph=None, visualization_setting=VisualizationSetting.NONE,
            **others) -> SamplePlan:
    """The plan of DiffusionLoss.sample(**the same keywords) for a diffusion of T timesteps, or the ValueError the call is
    rejected with.  What every keyword means is documented there.  Reads and advances no generator, takes no model: `model`,
    `t_emb_weights` and `show_bonds` may be among the keywords, so that both callers hand over one set, and are not looked at."""
    decided, passes, jump = check_options(noise=noise, condition=condition, symmetry=symmetry, seed=seed, fixed_cell=fixed_cell,
                                          use_graph=use_graph, visualization_setting=visualization_setting, **others)
    schedule, top, num_atoms_per_sample, num_samples_in_batch = _resolve_schedule(
        T, initial_state, z_table, condition, symmetry, lattice_system, num_atoms_per_sample, num_samples_in_batch, num_steps, timesteps)
    specs, num_atoms_per_sample, num_samples_in_batch, lattice_system = _resolve_symmetry(
        symmetry, num_atoms_per_sample, num_samples_in_batch, lattice_system, constant_atoms,
        (("condition", condition is not None), ("corrector_steps > 0", decided["corrector"] is not None),
         ("resample_passes > 1", passes > 1), (f"noise={noise!r}", noise != "philox")), decided["eta"])
    if condition is not None:
        num_atoms_per_sample, num_samples_in_batch = condition.resolve_batch(num_atoms_per_sample, num_samples_in_batch)
        condition.check_sampling(z_table, noise=noise, fixed_cell=fixed_cell, constant_species=constant_atoms is not None)
    elif num_atoms_per_sample is None or num_samples_in_batch is None:
        raise ValueError("num_atoms_per_sample and num_samples_in_batch are needed without a condition")
    B = int(num_samples_in_batch)
    xrd_guidance_mod.check_sampling(decided["xrd_guidance"], B=B)
    if decided["crystal_keys"] is not None:
        keyed_mod.validate_keys(decided["crystal_keys"], B, seed)
    lattice_systems.check(lattice_system, B, condition.lattice_known() if condition is not None else None)
    num_atoms = atom_counts(num_atoms_per_sample, B)
    N = int(num_atoms.sum())
    allow_rows, crystal_of = _resolve_species(elements, z_table, num_atoms, condition, constant_atoms)
    holds_state = initial_state is not None and isinstance(constant_atoms, bool)  # (True: the state's own species; False: none)
    if constant_atoms is not None and not holds_state and torch.as_tensor(constant_atoms).numel() != N:
        raise ValueError("constant_atoms must hold one class index per atom")
    steps, t_first, successor = _visited(schedule, top, max_steps)
    return SamplePlan(
        **decided, num_atoms_per_sample=num_atoms_per_sample, num_atoms=num_atoms, B=B, N=N,
        S=len(z_table) if z_table is not None else None, specs=specs, lattice_system=lattice_system, schedule=schedule, top=top,
        steps=steps, t_first=t_first, successor=successor, resampling=(passes, jump, schedule) if passes > 1 else None,
        allow_rows=allow_rows, crystal_of=crystal_of, use_graph=len(steps) * passes >= 200 if use_graph is None else bool(use_graph),
        stops=[j for j in range(1, len(steps)) if frame_after(visualization_setting, steps[j])],
        # (the successor of the last step is the timestep it produces)
        events=rs.plan(steps, (steps[-1] - 1 if schedule is None else successor[steps[-1]]) if steps else 0, passes, jump))
