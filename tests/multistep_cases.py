"""Cases shared by the multistep tests (test_multistep_cpu.py, test_gpu_multistep_sampling.py): the analytic Gaussian case, the
schedules of the step tests with the branch every move takes, and the model's float32 tables held as float64."""
import numpy as np

from arreau_amd.diffusion import multistep as ms, respacing

T = 100
MEAN, VAR = 0.3, 0.25           # the data distribution of the analytic case, per component
X_START, L_START = 0.9, 1.7     # where its trajectories start (positions unwrapped)
COUNTS = [1, 3, 8, 20, 2]       # one atom per crystal; a ragged tail that is no multiple of four waves; under three crystals per lattice block
CODES = [0, 1, 2, 0, 1]         # the lattice-system tie of the tied cases

# Three consecutive steps each.  Positions, on the geometric sigma ladder r is the ratio of the level differences: 39 / 10 = 3.9
# for 60 -> 50 after 99 (first order) and 10 / 5 = 2 for 50 -> 45 after 60 (second order).  Lengths, on the cosine schedule at
# T = 100: r = 12.0 for 60 -> 50 after 99 (first order), 2.03 for 50 -> 45 after 60 (second), 1.71 / 1.41 at the top (second),
# 0.59 for 2 -> 1 after 3 (second).  The first move of a run has no history and the move to level 0 is first order.
STEP_SCHEDULES = {
    (99, 98, 97, 96): dict(positions=[False, True, True], lengths=[False, True, True]),
    (99, 60, 50, 45): dict(positions=[False, False, True], lengths=[False, False, True]),
    (3, 2, 1, 0): dict(positions=[False, True, False], lengths=[False, True, False]),
}


def tables(T=T):
    """(ve_sigmas, vp_alpha_bars, vp_betas) of a model with T timesteps: the float32 tables as float64."""
    import torch
    from oracle import diffusion as OD
    sig = OD.ve_sigmas(T, 0.001, 1.0, dtype=torch.float32).double().numpy()
    ab, betas, _ = OD.vp_schedule(T, dtype=torch.float32)
    return sig, ab.double().numpy(), betas.double().numpy()


def analytic_errors(K, T=T):
    """The analytic case on the project's evenly spaced schedule of K steps: |final - probability-flow image of the start| of
    the multistep and of the eta = 0 trajectory, as (positions multistep, positions eta0, lengths multistep, lengths eta0)."""
    sig, ab, _ = tables(T)
    sched = respacing.respaced_timesteps(T, K)
    x, l = np.array([X_START]), np.array([L_START])
    want_x = ms.gaussian_position_flow(sig, MEAN, VAR, x, sched[0], 0)
    want_l = ms.gaussian_length_flow(ab, MEAN, VAR, l, sched[0], 0)
    out = []
    for multistep in (True, False):
        got_x, _ = ms.position_trajectory(sig, sched, x, ms.gaussian_eps(sig, MEAN, VAR), multistep=multistep)
        out.append(float(np.abs(got_x - want_x)[0]))
    for multistep in (True, False):
        got_l, _ = ms.length_trajectory(ab, sched, l, ms.gaussian_x0(ab, MEAN, VAR), multistep=multistep)
        out.append(float(np.abs(got_l - want_l)[0]))
    return tuple(out)
