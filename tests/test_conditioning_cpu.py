"""Conditioned sampling, host side (no GPU): the SampleCondition template form, its validation (which runs before the engine
is touched), the host matrix_to_params, and generate.py's template tiling and rank slicing."""
import numpy as np
import pytest
import torch

from oracle import geometry as OG
from arreau_amd.diffusion.conditioning import SampleCondition
from arreau_amd.diffusion.diffusion_loss import SampleResult
from arreau_amd.diffusion.inference.process_generated_crystals import (load_sample_results_from_hdf5,
                                                                      save_sample_results_to_hdf5)
from arreau_amd.diffusion.lattice_helpers import matrix_to_params
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable
from arreau_amd import generate

ZT = AtomicNumberTable([1, 6, 8, 14, 2001])


def _template(counts=(3, 5, 2), seed=0):
    rng = np.random.RandomState(seed)
    B, N = len(counts), sum(counts)
    lengths = torch.tensor(rng.uniform(3, 7, (B, 3)), dtype=torch.float64)
    angles = torch.tensor(np.deg2rad(rng.uniform(70, 110, (B, 3))), dtype=torch.float64)
    lattice = OG.lattice_from_params(lengths, angles).numpy()
    na = np.asarray(counts, dtype=np.int64)
    return SampleResult(frac_x=rng.uniform(0, 1, (N, 3)), atomic_numbers=rng.choice([1, 6, 8, 14], N).astype(np.float64),
                        lattice=lattice, num_atoms=na, idx_start=np.cumsum(na) - na)


class _NoEngine:
    """A model whose engine must not be reached: every ValueError below comes from validation first."""
    def engine(self):
        raise AssertionError("the engine was touched before the condition was validated")


def _sample(cond, **kw):
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = 100
    return dl.sample(model=_NoEngine(), z_table=ZT, condition=cond, **kw)


def test_from_sample_result_on_the_npz_wire_format(tmp_path):
    res = _template()
    path = str(tmp_path / "crystals.npz")
    save_sample_results_to_hdf5(res, path)
    loaded = load_sample_results_from_hdf5(path)
    pm = np.zeros(10, dtype=bool)
    pm[[0, 4, 9]] = True
    c = SampleCondition.from_sample_result(loaded, fix_positions=pm, fix_species=True, fix_lattice=[True, False, True])
    assert c.B == 3 and c.N == 10 and c.num_atoms.tolist() == [3, 5, 2]
    assert c.positions_known().tolist() == pm.tolist() and c.species_known().all()
    assert c.lattice_known().tolist() == [True, False, True]
    np.testing.assert_array_equal(c.frac_x, res.frac_x)
    np.testing.assert_array_equal(c.lattice, res.lattice)
    c.validate(ZT)
    # generate.load_template: masks in the file win, --fix fills in the absent ones
    np.savez(str(tmp_path / "masked.npz"), frac_x=res.frac_x, atomic_numbers=res.atomic_numbers, lattice=res.lattice,
             idx_start=res.idx_start, num_atoms=res.num_atoms, position_mask=pm.astype(np.uint8))
    t = generate.load_template(str(tmp_path / "masked.npz"), generate.parse_fix("positions,lattice"))
    assert t.positions_known().tolist() == pm.tolist() and not t.species_known().any() and t.lattice_known().all()
    with pytest.raises(ValueError):
        generate.parse_fix("positions,cell")
    with pytest.raises(ValueError):
        SampleCondition.from_sample_result(res, fix_positions=np.ones(4, dtype=bool))


def test_host_matrix_to_params_against_the_oracle():
    rng = np.random.RandomState(3)
    B = 64
    lengths = torch.tensor(rng.uniform(1, 30, (B, 3)), dtype=torch.float64)
    angles = torch.tensor(np.deg2rad(rng.uniform(60, 120, (B, 3))), dtype=torch.float64)
    mats = OG.lattice_from_params(lengths, angles)
    mats = mats + torch.tensor(rng.normal(scale=0.1, size=(B, 3, 3)))  # general matrices as well
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # the oracle allocates its angle tensor in the default dtype
    try:
        l_o, a_o = OG.matrix_to_params(mats)
    finally:
        torch.set_default_dtype(prev)
    l, a = matrix_to_params(mats)
    np.testing.assert_allclose(l, l_o.numpy(), atol=1e-12, rtol=0)
    np.testing.assert_allclose(a, a_o.numpy(), atol=1e-12, rtol=0)
    # lattice_from_params of the parameters reproduces a matrix in the library's convention
    mats = OG.lattice_from_params(lengths, angles)
    l, a = matrix_to_params(mats.numpy())
    back = OG.lattice_from_params(torch.tensor(l), torch.tensor(a))
    np.testing.assert_allclose(back.numpy(), mats.numpy(), atol=1e-12, rtol=0)


def test_every_invalid_condition_raises_before_the_engine():
    res = _template()
    ok = SampleCondition.from_sample_result(res, fix_positions=True, fix_species=True, fix_lattice=True)
    ok.validate(ZT)
    bad_shape = SampleCondition.from_sample_result(res, fix_positions=True)
    bad_shape.frac_x = bad_shape.frac_x[:, :2]
    bad_mask = SampleCondition.from_sample_result(res, fix_positions=True)
    bad_mask.position_mask = bad_mask.position_mask[:-1]
    res_z = _template()
    res_z.atomic_numbers[2] = 26  # not in the z-table
    not_in_table = SampleCondition.from_sample_result(res_z, fix_species=True)
    res_m = _template()
    res_m.atomic_numbers[0] = 2001
    mask_state = SampleCondition.from_sample_result(res_m, fix_species=True)
    res_l = _template()
    res_l.lattice[1] = 0.0
    zero_length = SampleCondition.from_sample_result(res_l, fix_lattice=True)
    for cond in (bad_shape, bad_mask, not_in_table, mask_state, zero_length):
        with pytest.raises(ValueError):
            cond.validate(ZT)
        with pytest.raises(ValueError):
            _sample(cond)
    # unknown components are not read: an off-table species of an unmasked atom is fine
    sm = np.ones(10, dtype=bool)
    sm[2] = False
    SampleCondition.from_sample_result(res_z, fix_species=sm).validate(ZT)
    lat = SampleCondition.from_sample_result(res, fix_lattice=True)
    with pytest.raises(ValueError, match="fixed_cell"):
        _sample(lat, fixed_cell=True)
    for noise in ("reference", "device"):
        with pytest.raises(ValueError, match="philox"):
            _sample(ok, noise=noise)
    species = SampleCondition.from_sample_result(res, fix_species=True)
    with pytest.raises(ValueError, match="species"):
        _sample(species, constant_atoms=torch.zeros(10, dtype=torch.long))
    with pytest.raises(ValueError, match="num_samples_in_batch"):
        _sample(ok, num_samples_in_batch=4)
    with pytest.raises(ValueError, match="num_atoms_per_sample"):
        _sample(ok, num_atoms_per_sample=5)
    with pytest.raises(AssertionError, match="engine"):  # a valid condition gets as far as the engine
        _sample(ok, num_atoms_per_sample=[3, 5, 2], num_samples_in_batch=3)


def test_wrapper_refuses_constant_symbols_with_a_species_mask():
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    species = SampleCondition.from_sample_result(_template(), fix_species=True)
    with pytest.raises(ValueError, match="species"):
        PONITA_DIFFUSION.sample(object.__new__(PONITA_DIFFUSION), 5, 3, use_constant_atomic_symbols=["C"] * 5,
                                condition=species)


def test_template_tiling_and_rank_slicing():
    res = _template(counts=(3, 5, 2))
    c = SampleCondition.from_sample_result(res, fix_positions=True, fix_lattice=[True, False, True]).tile(3)
    assert c.B == 9 and c.num_atoms.tolist() == [3, 5, 2] * 3 and c.N == 30
    assert c.lattice_known().tolist() == [True, False, True] * 3
    np.testing.assert_array_equal(c.frac_x[10:20], res.frac_x)
    np.testing.assert_array_equal(c.lattice[6:9], res.lattice)
    for world in (1, 2, 4):
        covered = []
        for rank in range(world):
            pieces = generate.template_batches(c.B, 2, rank, world)
            assert all(0 < b - a <= 2 for a, b in pieces)
            covered += [i for a, b in pieces for i in range(a, b)]
        assert covered == list(range(c.B)), world  # contiguous, in crystal order, nothing twice
    part = c.slice(3, 5)  # template crystals 0 and 1 of the second tile
    assert part.num_atoms.tolist() == [3, 5]
    np.testing.assert_array_equal(part.frac_x, res.frac_x[:8])
    np.testing.assert_array_equal(part.lattice, res.lattice[:2])
    assert part.lattice_known().tolist() == [True, False]
    # the driver concatenates the per-batch results in crystal order
    seen = []

    def fake_sample(cond):
        seen.append(cond.num_atoms.tolist())
        return SampleResult(frac_x=cond.frac_x, atomic_numbers=np.ones(cond.N), lattice=cond.lattice, num_atoms=cond.num_atoms)

    out = generate.generate_from_template(fake_sample, c, num_crystals_per_batch=4)
    assert seen == [[3, 5, 2, 3], [5, 2, 3, 5], [2]]
    np.testing.assert_array_equal(out.frac_x, c.frac_x)
    assert out.num_atoms.tolist() == c.num_atoms.tolist()
    with pytest.raises(ValueError):
        c.tile(0)
