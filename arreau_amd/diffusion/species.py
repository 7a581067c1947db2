"""Species control of the sampler: per-crystal element sets and a species temperature (extension; the rules are stated in
include/arreau_hip.h, section "Species control"; arreau_sample_loop_species / arreau_reverse_step_species).

The D3PM species step may choose, per crystal, among an admitted set of classes only ("generate in a chemical system"), and its
Gumbel term is scaled by a temperature that can be turned down to 0, which makes the eta = 0 and multistep samplers functions of
the initial state in all three components.  Host side: element sets -> admission rows -> the packed words the kernels read, the
validation, and a float64 restatement of the rule for the tests.  No claim on sample quality is made."""
import math
import numpy as np

from .tools.atomic_number_table import SYMBOL_TO_Z, AtomicNumberTable

WORDS = 4          # uint32 words per admission row
MAX_CLASSES = 124  # the kernels' two classes per lane, S <= 124
D3PM_EPS = 1e-6


def validate_temperature(temperature) -> float:
    """The species temperature as a float: finite and >= 0, or ValueError."""
    try:
        tau = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"species_temperature must be a number >= 0, not {temperature!r}") from None
    if not math.isfinite(tau) or tau < 0.0:
        raise ValueError(f"species_temperature must be finite and >= 0, not {temperature!r}")
    return tau + 0.0  # (-0.0 -> 0.0)


def _is_atom(entry) -> bool:
    return isinstance(entry, (str, int, np.integer)) and not isinstance(entry, bool)


def _one_row(entry, z_table: AtomicNumberTable, what: str) -> np.ndarray:
    S = len(z_table)
    if entry is None:  # unrestricted: every class, the mask class included
        return np.ones(S, dtype=bool)
    if _is_atom(entry):
        raise ValueError(f"{what}: an element set is a collection of symbols and / or atomic numbers, not {entry!r}")
    row = np.zeros(S, dtype=bool)
    for e in entry:
        if isinstance(e, str):
            if e not in SYMBOL_TO_Z:
                raise ValueError(f"{what}: unknown element symbol {e!r}")
            z = SYMBOL_TO_Z[e]
        elif _is_atom(e):
            z = int(e)
        else:
            raise ValueError(f"{what}: {e!r} is neither an element symbol nor an atomic number")
        if z == AtomicNumberTable.MASK_ATOMIC_NUMBER or z not in z_table.zs:
            raise ValueError(f"{what}: element {e!r} (Z = {z}) is not in the model's table")
        row[z_table.z_to_index(z)] = True
    if not row.any():
        raise ValueError(f"{what}: an element set must not be empty")
    return row


def resolve_elements(elements, z_table: AtomicNumberTable, B: int) -> np.ndarray:
    """The admission rows, bool [B, S], of `elements`: one collection for the whole batch, or a list with one entry per crystal.
    An entry is None (unrestricted: all ones, the mask bit included) or a collection of symbols and / or atomic numbers; a
    restricted crystal gets its elements' class bits with the mask bit clear, so listing every element of the table asks only
    for "no atom ends as the mask state".  ValueError: an unknown symbol, an element the model's table does not hold, an empty
    set, a list of the wrong length."""
    S, B = len(z_table), int(B)
    if S > MAX_CLASSES:
        raise ValueError(f"species control takes at most {MAX_CLASSES} classes, the table has {S}")
    if elements is None:
        return np.ones((B, S), dtype=bool)
    if _is_atom(elements):
        raise ValueError(f"elements: a collection of symbols and / or atomic numbers is needed, not {elements!r}")
    entries = list(elements)
    per_crystal = any(e is None or isinstance(e, (list, tuple, set, frozenset, np.ndarray)) for e in entries)
    if not per_crystal:
        return np.tile(_one_row(entries, z_table, "elements"), (B, 1))
    if len(entries) != B:
        raise ValueError(f"elements: {len(entries)} entries for a batch of {B} crystals")
    return np.stack([_one_row(e, z_table, f"elements of crystal {b}") for b, e in enumerate(entries)]) if B else np.ones((0, S), bool)


def pack_rows(rows) -> np.ndarray:
    """bool [B, S] -> uint32 [B, 4]: class c is bit c & 31 of word c >> 5."""
    rows = np.asarray(rows, dtype=bool)
    if rows.ndim != 2 or rows.shape[1] > MAX_CLASSES:
        raise ValueError(f"admission rows must be [B, S] with S <= {MAX_CLASSES}")
    words = np.zeros((rows.shape[0], WORDS), dtype=np.uint32)
    for c in range(rows.shape[1]):
        words[:, c >> 5] |= rows[:, c].astype(np.uint32) << np.uint32(c & 31)
    return words


def unpack_rows(words, S: int) -> np.ndarray:
    """uint32 [B, 4] -> bool [B, S]; bits at or above S are ignored."""
    words = np.asarray(words).astype(np.uint32).reshape(-1, WORDS)
    c = np.arange(int(S))
    return ((words[:, c >> 5] >> (c & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def device_rows(rows, device):
    """The packed rows on `device` as the int32 tensor [B, 4] the engine takes (the bits of the uint32 words)."""
    import torch
    return torch.from_numpy(pack_rows(rows).view(np.int32).copy()).to(device).contiguous()


def check_rows(rows) -> None:
    """ValueError when a row admits no ordinary class (the last class is the mask state)."""
    rows = np.asarray(rows, dtype=bool)
    bad = np.nonzero(~rows[:, :-1].any(axis=1))[0]
    if bad.size:
        raise ValueError(f"species control: crystal {int(bad[0])} admits no ordinary class")


def check_held(rows, crystal, classes, held, what: str) -> None:
    """ValueError when a held species (classes[i] where held[i]) lies outside its crystal's row."""
    rows, crystal = np.asarray(rows, dtype=bool), np.asarray(crystal).reshape(-1)
    classes, held = np.asarray(classes).reshape(-1).astype(np.int64), np.asarray(held).reshape(-1).astype(bool)
    inside = (classes >= 0) & (classes < rows.shape[1])
    ok = np.zeros_like(held)
    ok[inside] = rows[crystal[inside], classes[inside]]
    bad = np.nonzero(held & ~ok)[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"{what}: atom {i} of crystal {int(crystal[i])} holds class {int(classes[i])}, outside the crystal's element set")


def admitted(rows, t: int) -> np.ndarray:
    """E(b, t) as bool [B, S]: the ordinary classes whose bit is set, and the mask class S - 1 -- always above t = 1, at t = 1 by
    its own bit."""
    out = np.array(rows, dtype=bool, copy=True)
    if t > 1:
        out[:, -1] = True
    return out


def species_step(q1t, qmats, logits, x_t, t: int, s: int, u, rows, crystal, temperature: float):
    """The species rule (steps 1-5) in float64 on the model's float32 tables: q1t [T, S, S] (Q_t^T), qmats [T, S, S] (Qbar_t),
    logits [N, S], x_t [N], the step from t to s, the uniforms u [N, S] (None at temperature 0), the admission rows bool [B, S]
    and the crystal of every atom.  Returns (class [N] int64, margin [N] float64): the margin between the two largest admitted
    values (inf where fewer than two compete)."""
    f64 = lambda v: np.asarray(v.detach().cpu() if hasattr(v, "detach") else v, dtype=np.float64)
    q1t, qmats, logits = f64(q1t), f64(qmats), f64(logits)
    x_t = np.asarray(x_t.detach().cpu() if hasattr(x_t, "detach") else x_t).astype(np.int64).reshape(-1)
    E = admitted(rows, t)[np.asarray(crystal).reshape(-1)]  # [N, S]
    with np.errstate(all="ignore"):
        l = np.where(E, logits, -np.inf)
        if t == 1:
            post = l
        else:
            mx = l.max(axis=1, keepdims=True)
            e = np.where(E, np.exp(l - mx), 0.0)
            p = e / e.sum(axis=1, keepdims=True)
            fact1 = q1t[t - 1, x_t, :] if s == t - 1 else qmats[t - s - 1][:, x_t].T
            fact2 = p @ qmats[s - 1]
            post = np.where(E, np.log(fact1 + D3PM_EPS) + np.log(fact2 + D3PM_EPS), -np.inf)
        value = post
        tau = validate_temperature(temperature)
        if tau > 0.0:
            g = -np.log(-np.log(np.clip(f64(u), D3PM_EPS, 1.0)))
            value = post + (tau * (1.0 if t != 1 else 0.2)) * g
        value = np.where(E & (value > -np.inf), value, -np.inf)  # (a NaN does not compete)
    cls = np.argmax(value, axis=1)  # first index on ties
    none = ~(value > -np.inf).any(axis=1)
    cls[none] = np.argmax(E[none], axis=1)  # the lowest admitted class
    top = -np.sort(-value, axis=1)[:, :2]
    with np.errstate(all="ignore"):
        margin = top[:, 0] - top[:, 1] if value.shape[1] > 1 else np.full(len(cls), np.inf)
    margin = np.where(np.isnan(margin), np.inf, margin)
    return cls.astype(np.int64), margin


def describe(rows_one, z_table: AtomicNumberTable) -> str:
    """One row as text: the admitted atomic numbers (the mask state as its 2001)."""
    return ", ".join(str(z_table.zs[c]) for c in np.nonzero(np.asarray(rows_one, dtype=bool))[0])
