"""Cases shared by the species-control tests (test_species_cpu.py, test_gpu_species_sampling.py): the batch, the step pairs,
the admission rows of both models and the seeded inputs of one step.  The scaffolding is tests/sampling_helpers.py's (Case,
S = 12, T = 100, fused_model, any_model); the second model is make_synthetic_model(S=124, num_timesteps=100), two classes per
lane."""
import numpy as np
import torch

from tests.sampling_helpers import S as S12, T

COUNTS = [4, 7, 2, 150]  # ragged, one crystal above 128 atoms
PAIRS = [(99, 80), (50, 10), (7, 1), (2, 1), (1, 0), (60, 59)]  # strided, onto 1, stride 1 onto 1, the last step, stride 1
TAUS = [0.0, 0.5, 1.0]
MARGIN = 1e-4  # a class may differ from the float64 arg-max only where the two best admitted values are closer than this
S124 = 124
MODEL_SEED = 4321

# per crystal: a set of admitted ordinary classes, or None (unrestricted: all ones, the mask bit included)
ROWS = {
    "S12": {"mixed": [{3}, {0, 5, 10}, None, set(range(S12 - 1))]},
    "S124": {
        # sets that touch all four words
        "words": [{1, 40, 70, 100, 122}, {0, 31, 32, 95, 96}, None, {5, 63, 64, 99, 122}],
        # single-class rows at the word and lane boundaries
        "single-a": [{31}, {32}, {63}, {64}],
        "single-b": [{122}, {64}, {31}, {1, 40, 70, 100, 122}],
    },
}
SIZES = {"S12": S12, "S124": S124}
CASES = [(name, group) for name in ROWS for group in ROWS[name]]


def rows_of(sets, S):
    """bool [B, S] of a list of sets / None."""
    out = np.zeros((len(sets), S), dtype=bool)
    for b, e in enumerate(sets):
        if e is None:
            out[b] = True
        else:
            out[b, sorted(e)] = True
    return out


def crystal_index(counts=COUNTS):
    return np.repeat(np.arange(len(counts)), counts)


def tables(S, T=T):
    """(q_one_step_transposed, q_mats) of a model with S classes: the float32 tables (the mask chain depends on S and T only)."""
    from oracle import diffusion as OD
    return OD.d3pm_buffers(T, S, dtype=torch.float32)


def step_inputs(S, t, counts=COUNTS, seed=0):
    """The network outputs, draws and x_t classes of one step on the host: x_t runs over every class in the large crystal (the
    mask class and classes outside the crystal's set included) and starts with the mask class."""
    g = torch.Generator().manual_seed(7000 + 13 * t + S + seed)
    B, N = len(counts), sum(counts)
    eps = torch.randn(N, 3, generator=g) * 0.3
    logits = torch.randn(N, S, generator=g) * 2.0
    len0 = torch.rand(B, 3, generator=g) + 0.5
    z_l, z_f, u = torch.randn(B, 3, generator=g), torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g)
    x_t = torch.randint(0, S, (N,), generator=g)
    x_t[0] = S - 1
    x_t[N - S:] = torch.arange(S)
    return eps, logits, len0, z_l, z_f, u, x_t
