"""All six per-crystal instruments at once (arreau_amd/diffusion/instruments.py): sample() with every keyword against one call per
keyword, and the two command lines with every flag, each a fresh process.  Needs an MI355X: `-m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd.diffusion.instruments import INSTRUMENTS
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("metrics", "uniqueness", "symmetry", "reduced", "symmetrized", "match")
LABELS = ("screen", "unique", "symmetry", "cell reduction", "symmetrize", "match")  # what a summary line starts with, in table order


def _sample(m, **kw):
    torch.manual_seed(3)
    np.random.seed(3)
    return m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)


def test_all_keywords_at_once_equal_one_keyword_each(fused_model):
    m, _ = fused_model
    plain = _sample(m)
    assert all(getattr(plain, f) is None for f in FIELDS)
    asked = dict(screen=True, unique=True, find_symmetry=True, reduce_cell=True, symmetrize=True, match_to=plain)  # three targets: paired
    assert tuple(asked) == tuple(e.keyword for e in INSTRUMENTS)
    every = _sample(m, **asked)
    for e in INSTRUMENTS:
        one = _sample(m, **{e.keyword: asked[e.keyword]})
        for r in (one, every):
            assert np.array_equal(r.frac_x, plain.frac_x) and np.array_equal(r.lattice, plain.lattice), e.keyword
            assert np.array_equal(r.atomic_numbers, plain.atomic_numbers), e.keyword
        assert [f for f in FIELDS if getattr(one, f) is not None] == [e.field]
        alone, together = getattr(one, e.field), getattr(every, e.field)
        assert set(alone) == set(together) >= set(e.keys), e.keyword
        for k, v in alone.items():
            w = together[k]
            assert v.dtype == w.dtype and v.shape == w.shape, (e.keyword, k)
            assert np.array_equal(v, w, equal_nan=v.dtype.kind == "f"), (e.keyword, k)


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


@pytest.fixture(scope="module")
def files(fused_model, tmp_path_factory):
    """A checkpoint, a file of five target crystals of four atoms, and the names of the two outputs."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results
    d = tmp_path_factory.mktemp("instruments")
    m, _ = fused_model
    torch.manual_seed(7)
    np.random.seed(7)
    targets = save_sample_results_to_hdf5(concat_results([m.sample(4, 5, seed=11, max_steps=6)]), str(d / "targets.npz"))  # (+ idx_start)
    ckpt = save_lightning_checkpoint(str(d / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    return dict(ckpt=ckpt, targets=targets, generated=str(d / "out" / "crystals.npz"), screened=str(d / "out" / "screened.npz"))


def _heads(text):
    """'screen rank 0', 'screen total', ..., 'wrote': what every printed line starts with."""
    return [line.split(":")[0] if not line.startswith("wrote ") else "wrote" for line in text.splitlines()]


def test_generate_with_every_flag(files):
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    text = _child(["arreau_amd.generate", "--model_path", files["ckpt"], "--num_crystals", "5", "--batch", "4", "--num_atoms", "4", "--num_steps", "10",
                   "--seed", "5", "--screen", "--unique", "--find_symmetry", "--reduce_cell", "--symmetrize", "--match_to", files["targets"],
                   "--out", files["generated"]], 300)
    assert _heads(text) == [f"{label} {who}" for label in LABELS for who in ("rank 0", "total")] + ["wrote"], text
    res = load_sample_results_from_hdf5(files["generated"])
    assert len(res.num_atoms) == 5 and [f for f in FIELDS if getattr(res, f) is None] == []
    for e in INSTRUMENTS:
        assert set(getattr(res, e.field)) >= set(e.keys) and all(len(getattr(res, e.field)[k]) == 5 for k in e.keys if k not in e.atom_keys)


def test_screen_with_every_flag(files):
    """On the file of test_generate_with_every_flag.  `python -m arreau_amd.screen` takes the file as one set, so duplicate detection
    prints its total alone; and after --reduce_cell / --symmetrize `--out` holds THOSE crystals with the reduced_*, symmetrized_* and
    match_* arrays -- the screen_*, unique_* and sym_* arrays describe the cells as given and are not written to it."""
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    assert os.path.exists(files["generated"]), "needs the file test_generate_with_every_flag writes"
    text = _child(["arreau_amd.screen", files["generated"], "--unique", "--find_symmetry", "--reduce_cell", "--symmetrize", "--match_to",
                   files["targets"], "--out", files["screened"]], 120)
    want = [f"{label} {who}" for label in LABELS for who in ("rank 0", "total") if (label, who) != ("unique", "rank 0")]
    assert _heads(text) == want + ["wrote"], text
    res = load_sample_results_from_hdf5(files["screened"])
    assert len(res.num_atoms) == 5 and [f for f in FIELDS if getattr(res, f) is not None] == ["reduced", "symmetrized", "match"]
    for e in INSTRUMENTS[3:]:
        assert set(getattr(res, e.field)) == set(e.keys) and all(len(getattr(res, e.field)[k]) == 5 for k in e.keys if k not in e.atom_keys)
    assert np.array_equal(res.frac_x, res.symmetrized["frac_x"]) and np.array_equal(res.num_atoms, res.reduced["num_atoms"])
