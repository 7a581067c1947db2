"""Keyed sampling: a crystal is a function of (seed, key), not of its batch (an extension; rules in include/arreau_hip.h, "keyed
sampling", restated here).

`sample(..., seed=s, crystal_keys=keys)` gives crystal b a random stream of its own:

  1. stream seed.  For a key 0 <= key < 2^63,  s_b = stream_seed(s, key_b) = w0 | w1 << 32  with w0, w1 words 0 and 1 of
     philox4x32_10(counter = (key lo, key hi, STREAM_SEED_TAG, 0), key = (seed lo, seed hi)), in exact integer arithmetic on the
     host.  (seed 5, key 1) and (seed 6, key 0) are different streams.
  2. draws of the loop.  Wherever the Philox loop draws (seed, t, kind, element, word3) the keyed loop draws
     (s_b, t, kind, element', word3), element' counted within the crystal: 3 a + d for positions (kinds 1, 3, 5, 6), d for
     lengths (kinds 0, 4, 7), a S + c for species (kinds 2, 8), a the atom's index in its crystal.  Kinds and word3 keep their
     meaning.
  3. initial state.  Kinds 13 (normal [3], lengths), 14 (normal [n,3], positions), 15 (uniform, the j-th uniform of the crystal's
     angle draw) at counter timestep 0; the host formulas of draw_initial_state are applied to them as to the generators' values.
     The host's global generators are neither read nor advanced.
  4. hence crystal b's state after any number of steps is a function of (model, options, seed, key_b, its atom count, its own
     inputs): within one score arithmetic bitwise independent of the other crystals, of its index and of the cut into calls.
  5. limits.  Batches on different sides of the score network's basis-form threshold (or with and without ARREAU_CROSS_FP8) agree
     to the bound of the network's batch-independence test, not bitwise; the re-run of a batch after an fp16x3 overflow is a
     decision about the whole batch.

numpy only at import.  The pure-Python Philox below restates the raw words and the uniforms for the tests; the normals are the
device's Box-Muller of words 0 and 1 (arreau_philox_fill_crystals)."""
from typing import Callable, Optional, Sequence

import numpy as np

STREAM_SEED_TAG = 0x4B455953  # "KEYS": counter word 2 of the stream-seed call (csrc/philox.h)
KIND_INIT_LENGTHS, KIND_INIT_FRAC, KIND_INIT_ANGLES = 13, 14, 15
KEY_LIMIT = 2 ** 63
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): the four output words of counter (c0, c1, c2, c3) under key (k0, k1)."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def stream_seed(seed: int, key: int) -> int:
    """Rule 1: the 64-bit stream seed of (seed, key)."""
    seed, key = int(seed) & (2 ** 64 - 1), int(key)
    if not 0 <= key < KEY_LIMIT:
        raise ValueError("a crystal key must lie in 0..2^63-1")
    w = philox4x32_10((key & _M32, key >> 32, STREAM_SEED_TAG, 0), (seed & _M32, seed >> 32))
    return w[0] | (w[1] << 32)


def stream_seeds(seed: int, keys) -> np.ndarray:
    """stream_seed of every key, uint64 [B]."""
    return np.array([stream_seed(seed, int(k)) for k in np.asarray(keys).reshape(-1)], dtype=np.uint64)


def device_seeds(streams: np.ndarray, device):
    """The table the keyed exports take: the uint64 stream seeds as the bits of a contiguous int64 tensor [B] on `device`."""
    import torch
    return torch.as_tensor(np.asarray(streams, dtype=np.uint64).view(np.int64), device=device).contiguous()


def raw_words(stream: int, timestep: int, kind: int, element: int, word3: int = 0):
    """Rule 2: the four raw words of the draw (stream seed, timestep, kind, element, word3)."""
    stream = int(stream)
    return philox4x32_10((element, timestep, kind, word3), (stream & _M32, stream >> 32))


def uniform(stream: int, timestep: int, kind: int, element: int, word3: int = 0) -> float:
    """The uniform in [0, 1) of a draw: the top 24 bits of word 0 (exact in float32 and float64)."""
    return (raw_words(stream, timestep, kind, element, word3)[0] >> 8) / 16777216.0


def angle_uniforms(stream: int) -> Callable[[float, float], float]:
    """Rule 3: np.random.uniform's stand-in for one crystal's angle draw -- the j-th call returns low + (high - low) u_j in
    float64, u_j the kind-15 uniform of element j."""
    j = [0]

    def draw(low, high):
        u = uniform(stream, 0, KIND_INIT_ANGLES, j[0])
        j[0] += 1
        return low + (high - low) * u
    return draw


def validate_keys(crystal_keys, B: Optional[int], seed, noise: str = "philox") -> np.ndarray:
    """The keys of a keyed call as int64 [B], or ValueError: integers in 0..2^63-1, one per crystal (B None: any count), no key
    twice, a seed given, noise='philox'.  Touches no generator."""
    if noise != "philox":
        raise ValueError("crystal_keys need noise='philox' (the host-noise modes draw in batch order)")
    if seed is None:
        raise ValueError("crystal_keys need a seed: a crystal is a function of (seed, key)")
    try:
        raw = [k for k in (crystal_keys.tolist() if hasattr(crystal_keys, "tolist") else list(crystal_keys))]
    except TypeError:
        raise ValueError("crystal_keys must be a sequence of integers, one per crystal") from None
    keys = []
    for k in raw:
        if isinstance(k, (bool, float)) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"crystal_keys must be integers, got {k!r}")
        if not 0 <= int(k) < KEY_LIMIT:
            raise ValueError(f"crystal key {int(k)} lies outside 0..2^63-1")
        keys.append(int(k))
    if B is not None and len(keys) != int(B):
        raise ValueError(f"crystal_keys holds {len(keys)} keys for a batch of {int(B)} crystals")
    if len(set(keys)) != len(keys):
        raise ValueError("crystal_keys holds a key twice: two crystals of a batch would be the same crystal")
    return np.array(keys, dtype=np.int64)


def slot_key(slot: int, attempt: int, num_crystals: int) -> int:
    """The key of output slot `slot` of a run of `num_crystals` on its attempt `attempt` (0: the first):
    attempt * num_crystals + slot."""
    slot, attempt, num_crystals = int(slot), int(attempt), int(num_crystals)
    if not (0 <= slot < num_crystals and attempt >= 0):
        raise ValueError("slot_key: slot must lie in 0..num_crystals-1 and attempt be >= 0")
    return attempt * num_crystals + slot


def parse_keys(text: str, num_crystals: int):
    """'17,4711' -> [17, 4711]: the slots of a run of num_crystals to regenerate; ValueError for one out of range or given twice."""
    try:
        slots = [int(p) for p in (part.strip() for part in text.split(",")) if p]
    except ValueError:
        raise ValueError("--keys takes comma-separated integers") from None
    if not slots:
        raise ValueError("--keys needs at least one slot")
    bad = [s for s in slots if not 0 <= s < int(num_crystals)]
    if bad:
        raise ValueError(f"--keys: slot(s) {bad[:8]} lie outside 0..{int(num_crystals) - 1}")
    if len(set(slots)) != len(slots):
        raise ValueError("--keys: a slot is given twice")
    return slots


def template_key(j: int, n_templates: int, samples_per_template: int) -> int:
    """The key of crystal j of a template set tiled samples_per_template times (order t0, t1, ..., t0, t1, ...): the template's
    index in the file times samples_per_template plus the copy."""
    j, n, K = int(j), int(n_templates), int(samples_per_template)
    if not (n >= 1 and K >= 1 and 0 <= j < n * K):
        raise ValueError("template_key: j must lie in 0..n_templates * samples_per_template - 1")
    return (j % n) * K + j // n


def fill_slots(sample_keys: Callable, slots: Sequence[int], num_crystals: int, batch: int = 256,
               valid_of: Optional[Callable] = None, max_rounds: int = 1):
    """The keyed driver's arithmetic on a rank's share `slots` of the output slots: round a (0, 1, ..) samples every slot that is
    still open under slot_key(slot, a, num_crystals), in sub-batches of at most `batch` keys through sample_keys(keys) -> result,
    and a slot keeps its first valid attempt (valid_of(result) -> bool per crystal; None: every crystal is valid and one round
    runs).  Since a crystal is a function of its key alone, the outcome does not depend on world_size or batch.
    Returns (accepted, attempts): accepted a list of (slot, key, result, index in result) in slot order, attempts the list of every
    (result, valid array, keys) in sampling order.  Slots still open after max_rounds are absent from `accepted`: a shortfall."""
    rounds = 1 if valid_of is None else int(max_rounds)
    if rounds < 1:
        raise ValueError(f"max_rounds must be >= 1, got {max_rounds}")
    open_slots = list(slots)
    done, attempts = {}, []
    for a in range(rounds):
        if not open_slots:
            break
        still = []
        for s in range(0, len(open_slots), int(batch)):
            part = open_slots[s:s + int(batch)]
            keys = [slot_key(k, a, num_crystals) for k in part]
            res = sample_keys(keys)
            ok = np.ones(len(part), dtype=bool) if valid_of is None else np.asarray(valid_of(res), dtype=bool).reshape(-1)
            attempts.append((res, ok, keys))
            for i, (slot, key) in enumerate(zip(part, keys)):
                if ok[i]:
                    done[slot] = (slot, key, res, i)
                else:
                    still.append(slot)
        open_slots = still
    return [done[s] for s in sorted(done)], attempts
