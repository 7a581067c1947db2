"""What the per-crystal analysis modules share (screening.py, uniqueness.py, symmetry_search.py, cell_reduction.py, symmetrize.py,
structure_match.py; their kernels share arreau_amd/csrc/crystal_dev.h in the same way): the check and the upload of a device batch,
`resolve`, the pieces of their statistics and summary lines, and the numpy pieces of the restatements.  Needs numpy alone at import;
torch is imported where a device is used."""
import numpy as np

STAGED_ATOMS = 256  # crystals of up to this many atoms keep their per-atom data in LDS (crystal_dev.h: CRYSTAL_LDS_ATOMS)
F32 = np.float32


def check_batch(caller, frac, lattice, offsets, types, types_optional=False):
    """The device batch of an entry point: frac [N,3] float32, lattice [B,3,3] float32, offsets [B+1] int32 and types [N] int32
    (may be None where it is optional), contiguous on one cuda device.  Returns (device, B, N)."""
    import torch
    dev = frac.device
    B, N = int(lattice.shape[0]), int(frac.shape[0])
    want = [("frac", frac, (N, 3), torch.float32), ("lattice", lattice, (B, 3, 3), torch.float32), ("offsets", offsets, (B + 1,), torch.int32)]
    for name, t, shape, dtype in want + ([] if types is None and types_optional else [("types", types, (N,), torch.int32)]):
        if t is None or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous() or dev.type != "cuda":
            raise ValueError(f"{caller}: {name} must be a contiguous {dtype} tensor of shape {shape} on the cuda device of frac")
    return dev, B, N


def upload(result, device):
    """(frac, lattice, offsets, types) of a SampleResult (or a loaded crystals file) as device tensors: its float64 arrays cast to
    float32, its atomic numbers taken as species ids."""
    import torch
    num_atoms = np.asarray(result.num_atoms, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(num_atoms)]).astype(np.int32)
    dev = torch.device(device)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return (up(np.asarray(result.frac_x, dtype=np.float32).reshape(-1, 3)), up(np.asarray(result.lattice, dtype=np.float32).reshape(-1, 3, 3)),
            up(off), up(np.rint(np.asarray(result.atomic_numbers).reshape(-1)).astype(np.int32)))


def compact_ragged(offsets, n_out, *arrays):
    """Per-atom outputs laid out at the input's offsets, crystal b using its first n_out[b] slots, as a dense ragged batch:
    (offsets_out [B+1] int64, [array rows of the used slots, in order])."""
    offsets, n_out = np.asarray(offsets, dtype=np.int64).reshape(-1), np.asarray(n_out, dtype=np.int64).reshape(-1)
    assert offsets.size == n_out.size + 1 and (n_out >= 0).all() and (n_out <= np.diff(offsets)).all()
    rows = np.concatenate([np.arange(a, a + k) for a, k in zip(offsets[:-1], n_out)] + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(n_out)]), [np.asarray(a)[rows] for a in arrays]


def resolve(value, cls, name):
    """sample(<name>=...): None / False -> None, True -> the defaults cls(), an instance of cls -> itself."""
    if value is None or value is False:
        return None
    if value is True:
        return cls()
    if isinstance(value, cls):
        return value
    raise ValueError(f"{name} must be None, True or a {cls.__name__}, got {value!r}")


def to_numpy(result):
    """A dict of device tensors (and whatever else it holds) as host numpy arrays (synchronises)."""
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in result.items()}


def crystal_arrays(frac_x, lattice, atomic_numbers, num_atoms):
    """The five arrays of a crystals file: frac_x and lattice float64, atomic_numbers, num_atoms, idx_start."""
    num_atoms = np.asarray(num_atoms, dtype=np.int64)
    return {"frac_x": np.asarray(frac_x, dtype=np.float64), "lattice": np.asarray(lattice, dtype=np.float64),
            "atomic_numbers": np.asarray(atomic_numbers), "num_atoms": num_atoms, "idx_start": np.concatenate([[0], np.cumsum(num_atoms)[:-1]])}


# ---------------------------------------------------------------------------------- statistics and summary lines: the shared pieces
def describe(flags, names) -> str:
    """'CELL|EMPTY' for the set bits of `flags` among names ((bit, name), ...); 'ok' for none."""
    names = [name for bit, name in names if int(flags) & bit]
    return "|".join(names) if names else "ok"


def rank_of(rank):
    """The `rank` entry of a statistics dict: an int, or "total"."""
    return rank if rank == "total" else int(rank)


def flag_counts(flags, names):
    """{name: crystals with that bit set} of flags [B] int64."""
    return {name: int(((flags & bit) != 0).sum()) for bit, name in names}


def who(st) -> str:
    """'total' or 'rank 3': whose statistics a summary line reports."""
    return "total" if st["rank"] == "total" else f"rank {st['rank']}"


def some(counts, sep=" ") -> str:
    """'CELL 2, EMPTY 1' of the non-zero entries of a {name: count} dict ('none' without any)."""
    return ", ".join(f"{k}{sep}{v}" for k, v in counts.items() if v) or "none"


def summary_lines(parts, format_stats, total_stats):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    parts = sorted(parts, key=lambda p: p["rank"])
    return [format_stats(p) for p in parts] + [format_stats(total_stats(parts))]


def inputs(frac, lattice, counts, types):
    """The restatements' inputs as the kernels see them: frac [N,3] and lattice [B,3,3] float32, counts a list of ints, types
    int64 [N] or None, and `first` [B+1], the crystals' first atoms."""
    frac = np.ascontiguousarray(frac, dtype=F32).reshape(-1, 3)
    lattice = np.ascontiguousarray(lattice, dtype=F32).reshape(-1, 3, 3)
    counts = [int(n) for n in counts]
    assert sum(counts) == frac.shape[0] and len(counts) == lattice.shape[0]
    types = None if types is None else np.asarray(types, dtype=np.int64).reshape(-1)
    return frac, lattice, counts, types, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def cell_f32(L, search_radius, min_volume, max_shells):
    """Volume, shells and the CELL decision of one finite cell [3,3] float32: (volume, q [3] float32, cell_bad)."""
    a = [L[0], L[1], L[2]]
    cross = lambda u, v: np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=F32)
    c = [cross(a[1], a[2]), cross(a[2], a[0]), cross(a[0], a[1])]
    det = (a[0][0] * c[0][0] + a[0][1] * c[0][1]) + a[0][2] * c[0][2]
    vol = np.abs(det)
    with np.errstate(all="ignore"):
        q = np.array([F32(search_radius) / (vol / np.sqrt((ck[0] * ck[0] + ck[1] * ck[1]) + ck[2] * ck[2])) for ck in c], dtype=F32)
    bad = (not vol >= F32(min_volume)) or (not np.isfinite(vol)) or any(not qk <= F32(max_shells) for qk in q)
    return vol, q, bad


def cell_f64(L, search_radius):
    """Volume and shell quotients q [3] = search_radius / h_k of one finite cell [3,3] float64 (inf for a cell without volume)."""
    c = np.array([np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])])
    vol = abs(float(np.dot(L[0], c[0])))
    with np.errstate(all="ignore"):
        q = search_radius * np.linalg.norm(c, axis=1) / vol if vol > 0 else np.full(3, np.inf)
    return vol, q


def shift_table(nk):
    """[M,3] integer images in lexicographic order and the index of (0, 0, 0)."""
    g = np.stack(np.meshgrid(*[np.arange(-k, k + 1) for k in nk], indexing="ij"), -1).reshape(-1, 3)
    return g, int(((nk[0] * (2 * nk[1] + 1)) + nk[1]) * (2 * nk[2] + 1) + nk[2])


def positions_and_shifts(f, L, nk, dtype):
    """(p [n,3], g [M,3], centre, s [M,3]) of one crystal in `dtype`: wrapped positions (w = f - floor(f), a result >= 1 becomes
    0), the image table of nk and its shift vectors; each a combination (c_0 L_0 + c_1 L_1) + c_2 L_2, in float32 one rounding
    per operation (numpy never contracts); the float64 restatements, which restate no operation order, take numpy's product."""
    w = (f - np.floor(f)).astype(dtype)
    w[w >= dtype(1)] = dtype(0)
    g, centre = shift_table(nk)
    rows = lambda c: c @ L if dtype == np.float64 else ((c[:, 0:1] * L[0][None] + c[:, 1:2] * L[1][None]) + c[:, 2:3] * L[2][None]).astype(dtype)
    return rows(w), g, centre, rows(g.astype(dtype))


def contacts(p, s, centre, dtype, chunk=1 << 19):
    """Every contact of one crystal in the rule's enumeration order: yields (i [K], j [K], m [K], d2 [K]) blocks; p [n,3]
    positions, s [M,3] shift vectors, both of `dtype`, every operation rounded to it."""
    n, M = p.shape[0], s.shape[0]
    iu, ju = np.triu_indices(n)  # row-major: lexicographic (i, j), i <= j
    step = max(1, chunk // M)
    for a in range(0, iu.size, step):
        i, j = iu[a:a + step], ju[a:a + step]
        disp = ((p[j][:, None, :] + s[None, :, :]).astype(dtype) - p[i][:, None, :]).astype(dtype)
        sq = (disp * disp).astype(dtype)
        d2 = ((sq[..., 0] + sq[..., 1]).astype(dtype) + sq[..., 2]).astype(dtype)
        m = np.broadcast_to(np.arange(M)[None, :], d2.shape)
        keep = (i != j)[:, None] | (m > centre)
        yield (np.broadcast_to(i[:, None], d2.shape)[keep], np.broadcast_to(j[:, None], d2.shape)[keep], m[keep], d2[keep])
