"""Restatements and inputs shared by tests/test_training_run_cpu.py and tests/test_gpu_training_run.py: Philox4x32-10 and the keyed
draw rules of arreau_diffusion_noise_keyed in numpy, the integer timestep rule, the binned reduction of a row table in float64,
and the hand-built crystals of the GPU tests.  Nothing here imports the library."""
from types import SimpleNamespace

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
KIND_T, KIND_Z_FRAC, KIND_U_TYPES, KIND_Z_LENGTHS = 9, 10, 11, 12

# Random123's known-answer vectors for philox4x32-10 (kat_vectors): (counter, key, result)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: ten rounds of two 32 x 32 -> 64 bit products, the key bumped by the Weyl
    constants between rounds.  Returns uint32 [..., 4]."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, element, timestep, kind, word3):
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10(element, timestep, kind, word3, seed & 0xFFFFFFFF, seed >> 32)


def uniform(w):
    """[0, 1) from the top 24 bits of word 0 (exact in float32 and float64)"""
    return (w[..., 0] >> np.uint32(8)).astype(np.float64) / 16777216.0


def normal(w):
    """Box-Muller of words 0 and 1, in float64: u1 in (0, 1], u2 in [0, 1)"""
    u1 = ((w[..., 0] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (w[..., 1] >> np.uint32(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def keyed_timestep(u24, copy, R, T):
    """t = 1 + ((copy 2^24 + u24) T) / (R 2^24) in integers; R > T is rejected (two copies would share a timestep)."""
    u24, copy, R, T = int(u24), int(copy), int(R), int(T)
    if not (1 <= R <= T and 0 <= copy < R and 0 <= u24 < 2 ** 24):
        raise ValueError("needs 1 <= R <= T, 0 <= copy < R and u24 < 2^24")
    return 1 + ((copy * 2 ** 24 + u24) * T) // (R * 2 ** 24)


def stratum(copy, R, T):
    """(lowest, highest) timestep copy `copy` of R can draw: the rule at u24 = 0 and at u24 = 2^24 - 1"""
    return keyed_timestep(0, copy, R, T), keyed_timestep(2 ** 24 - 1, copy, R, T)


def keyed_t(seed, crystal_id, copy, R, T):
    return keyed_timestep(int(words(seed, 0, 0, KIND_T, crystal_id)[0]) >> 8, copy, R, T)


def keyed_draws(seed, crystal_id, t, n, S):
    """The three draws of a crystal of n atoms at timestep t, float64: z_frac [n, 3], u_types [n, S], z_lengths [3]"""
    z_frac = normal(words(seed, np.arange(3 * n), t, KIND_Z_FRAC, crystal_id)).reshape(n, 3)
    u_types = uniform(words(seed, np.arange(n * S), t, KIND_U_TYPES, crystal_id)).reshape(n, S)
    z_len = normal(words(seed, np.arange(3), t, KIND_Z_LENGTHS, crystal_id))
    return z_frac, u_types, z_len


def gumbel_margin(q_row, u):
    """Winning minus runner-up score of D3PM.q_sample's arg-max for one atom, float64: log(q + 1e-6) - log(-log(clip(u, 1e-6, 1)))"""
    score = np.log(np.asarray(q_row, np.float64) + 1e-6) - np.log(-np.log(np.clip(u, 1e-6, 1.0)))
    top = np.sort(score)[-2:]
    return float(top[1] - top[0])


# ---- the crystals of the GPU tests: where a per-crystal reduction crosses a wave (64 | 65) and a 256-thread stride (256 | 257) ------
SIZES = (1, 2, 64, 65, 256, 257, 300)
IDS = (5, 0, 77, 4000000000, 12, 3, 901)  # dataset indices are arbitrary: not sorted, one above 2^31
# chosen on the CPU (float64 restatement): under it the seven timesteps include 1 and T = 10, and every atom's winning Gumbel score
# leads by more than 3e-3 at S = 90 and S = 124 (test 8 asserts the margin)
NOISE_SEED = 3


def crystals(S, sizes=SIZES, seed=3):
    """Hand-built crystals at 0.055 atoms / A^3 (triclinic cells, angles 75..105 degrees), species anywhere but the mask class.
    Returns a list of SimpleNamespace(X0 [n,3], A0 [n], L0 [3,3], num_atoms) in float64 / int64 numpy."""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        lengths = rng.uniform(0.8, 1.25, size=3)
        ca, cb, cg = np.cos(np.deg2rad(rng.uniform(75, 105, size=3)))
        sg = np.sqrt(1.0 - cg * cg)
        cx, cy = cb, (ca - cb * cg) / sg
        L = np.array([[lengths[0], 0.0, 0.0], [lengths[1] * cg, lengths[1] * sg, 0.0],
                      [lengths[2] * cx, lengths[2] * cy, lengths[2] * np.sqrt(1.0 - cx * cx - cy * cy)]])
        L *= (n / 0.055 / abs(np.linalg.det(L))) ** (1.0 / 3.0)
        out.append(SimpleNamespace(X0=rng.uniform(0, 1, size=(n, 3)), A0=rng.randint(0, S - 1, size=n).astype(np.int64), L0=L,
                                   num_atoms=int(n)))
    return out


def batch_of(items, ids, order=None):
    """The collated batch (numpy fields X0, A0, L0 [3B,3], num_atoms, index) of items[order]"""
    order = list(range(len(items))) if order is None else list(order)
    return SimpleNamespace(X0=np.concatenate([items[i].X0 for i in order]), A0=np.concatenate([items[i].A0 for i in order]),
                           L0=np.concatenate([items[i].L0 for i in order]), num_atoms=np.array([items[i].num_atoms for i in order]),
                           index=np.array([ids[i] for i in order], dtype=np.int64))


# ---- the binned reduction of a row table, float64 -----------------------------------------------------------------------------------
def bin_of(t, n_bins, T):
    return ((int(t) - 1) * int(n_bins)) // int(T)


def reduce_rows(sums, num_atoms, t, n_bins, T):
    """sums float [n, 4], num_atoms int [n], t int [n] -> (float64 [n_bins + 1, 4], int64 [n_bins + 1, 2] atoms and crystals,
    unwritten): rows with num_atoms <= 0 are skipped and counted; the last record is the total."""
    out, cnt, unwritten = np.zeros((n_bins + 1, 4)), np.zeros((n_bins + 1, 2), dtype=np.int64), 0
    for row, n, tt in zip(np.asarray(sums, dtype=np.float64), num_atoms, t):
        if n <= 0:
            unwritten += 1
            continue
        for q in (bin_of(min(max(int(tt), 1), T), n_bins, T), n_bins):
            out[q] += row
            cnt[q] += (int(n), 1)
    return out, cnt, unwritten


def set_loss(total_sums, total_counts):
    """The reference's batch loss of a set from its total record: (coord + 0.001 vb + ce) / N + lattice / (3 B)"""
    ef, vb, ce, el = (float(v) for v in total_sums)
    n, b = (int(v) for v in total_counts)
    return (ef + 0.001 * vb + ce) / n + el / (3 * b)
