"""The device-resident Langevin (BAOAB) driver (nequip_amd/integrations/md.py), ATen form on the CPU: the noise against the
published Philox known answers and its definition, the driver against the float64 restatement of tests/langevin_restatement.py
(whose docstring derives the bounds), plus the host logic that needs no GPU.  The kernels are tested in
tests/test_langevin_gpu.py."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import langevin_restatement as R
from nequip_amd.integrations import Langevin, NoseHoover, langevin_noise, units
from nequip_amd.integrations import md as md_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, T = 0.5 * R.FS, 300.0
FRICTION = 0.01 / R.FS

# Random123's kat_vectors for philox4x32-10: (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def make(n=7, seed=0, friction=FRICTION, temperature=T, fdtype=torch.float64, noise_seed=R.SEED, dt=DT, **kw):
    m, x, v = R.system(n, seed)
    drv = Langevin(R.torch_force_step(fdtype), torch.from_numpy(m), dt, temperature, friction, torch.from_numpy(x),
                   torch.from_numpy(v), seed=noise_seed, **kw)
    ref = R.Restated(R.restated_force("cpu", fdtype), m, dt, temperature, friction, x, v, seed=noise_seed)
    return drv, ref


def module_words(seed, step, count):
    z, w = langevin_noise(seed, step, count, "cpu", return_words=True)
    return z.numpy(), w.numpy().astype(np.uint64)


# ---- the noise --------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = [int(w[0]) for w in R.philox4x32_10(counter, key)]
        assert got == list(want), f"restatement, counter {counter}: {[hex(g) for g in got]}"
    # the module's generator at the counters its layout reaches: component i, step s, seed -> counter (i, 0, s lo, s hi)
    assert module_words(0, 0, 1)[1][0].tolist() == list(KNOWN_ANSWERS[0][2])
    all_ones = 2 ** 64 - 1
    count = 5
    got = module_words(all_ones, all_ones, count)[1]
    want = np.stack(R.philox4x32_10((np.arange(count), np.zeros(count), np.full(count, 0xFFFFFFFF), np.full(count, 0xFFFFFFFF)),
                                    (0xFFFFFFFF, 0xFFFFFFFF)), axis=1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("seed, step", [(0, 0), (R.SEED, 3), (2 ** 32 + 7, 1), (R.SEED, 2 ** 32 - 1), (R.SEED, 2 ** 32),
                                        (2 ** 64 - 1, 2 ** 64 - 1)])
def test_aten_noise_is_the_restatement(seed, step):
    for count in (1, 255, 258):
        z, w = module_words(seed, step, count)
        assert np.array_equal(w, R.words(seed, step, count)), "Philox words"
        assert np.array_equal(z, R.noise(seed, step, count)), "normals (the same numpy functions: the same bits)"
    assert langevin_noise(seed, step, 0).shape == (0,)


def test_noise_prefix_property_and_high_words():
    z258, z255 = R.noise(R.SEED, 4, 258), R.noise(R.SEED, 4, 255)
    assert np.array_equal(z258[:255], z255)
    assert torch.equal(langevin_noise(R.SEED, 4, 258)[:255], langevin_noise(R.SEED, 4, 255))
    # the high key word and the high counter word take part
    for words in (R.words, lambda *a: module_words(*a)[1]):
        base = words(7, 0, 16)
        assert not np.array_equal(words(2 ** 32 + 7, 0, 16), base), "seed >= 2^32 must change the words"
        lo, hi, zero = words(7, 2 ** 32 - 1, 16), words(7, 2 ** 32, 16), words(7, 0, 16)
        assert not np.array_equal(lo, hi) and not np.array_equal(hi, zero), "step 2^32 must differ from 2^32 - 1 and from 0"
        assert len({tuple(r) for r in np.concatenate([base, lo, hi]).tolist()}) == 48


def test_noise_moments():
    """409 650 values: the standard errors are 0.0016 (mean), 0.0022 (variance) and 0.0077 (kurtosis)."""
    z = np.concatenate([langevin_noise(R.SEED, s, 16386).numpy() for s in range(25)])
    assert z.shape == (409650,) and np.array_equal(z[:16386], R.noise(R.SEED, 0, 16386))
    mean, var = float(z.mean()), float(z.var())
    kurt = float(((z - mean) ** 4).mean() / var ** 2)
    print(f"mean {mean:.4f}, variance {var:.4f}, kurtosis {kurt:.4f}")
    assert abs(mean) < 0.01 and abs(var - 1.0) < 0.01 and abs(kurt - 3.0) < 0.05
    assert np.all(np.isfinite(z)) and np.abs(z).max() < 8.6


def test_noise_refusals():
    with pytest.raises(ValueError, match="seed"):
        langevin_noise(-1, 0, 4)
    with pytest.raises(ValueError, match="seed"):
        langevin_noise(2 ** 64, 0, 4)
    with pytest.raises(ValueError, match="step"):
        langevin_noise(0, -1, 4)
    with pytest.raises(ValueError, match="count"):
        langevin_noise(0, 0, -4)
    with pytest.raises(ValueError, match="backend='hip'"):
        langevin_noise(0, 0, 4, "cpu", backend="hip")


# ---- the driver -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ("f32", "f64"))
@pytest.mark.parametrize("n", (1, 7, 86))
def test_aten_driver_matches_the_restatement(n, fname):
    fdtype = {"f32": torch.float32, "f64": torch.float64}[fname]
    drv, ref = make(n, seed=n, fdtype=fdtype)
    assert not drv._hip and drv.forces.dtype == fdtype
    x0 = drv.positions.clone()
    for steps in (1, 24):
        drv.run(steps), ref.run(steps)
        R.assert_close(drv, ref, f"{n} atoms {fname}, after {ref.nsteps} steps")
    assert drv.nsteps == 25 and not torch.equal(drv.positions, x0)
    np.testing.assert_allclose(drv.forces.double().numpy(), ref.f, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(drv.potential_energy, float(R.energy_torch(torch.from_numpy(ref.x))), rtol=1e-9)
    assert drv.seed == R.SEED and drv.friction == FRICTION and not hasattr(drv, "nvt_bath")
    # the noise did something: another seed ends elsewhere
    other, _ = make(n, seed=n, fdtype=fdtype, noise_seed=R.SEED + 1)
    other.run(25)
    assert not torch.equal(other.positions, drv.positions)


@pytest.mark.parametrize("n", (7, 5462))
def test_friction_zero_is_velocity_verlet(n):
    drv, ref = make(n, seed=n, friction=0.0)
    assert (drv._c1, drv._c2) == (1.0, 0.0)
    x, v = R.velocity_verlet(R.restated_force("cpu"), ref.m, DT, ref.x, ref.v, 25)
    drv.run(25), ref.run(25)
    for got_x, got_v, what in ((drv.positions.numpy(), drv.velocities.numpy(), "driver"), (ref.x, ref.v, "restatement")):
        print(f"{what}: worst relative difference from velocity Verlet {np.max(np.abs(got_x - x) / np.abs(x)):.2e} (x), "
              f"{np.max(np.abs(got_v - v) / np.abs(v)):.2e} (v)")
        np.testing.assert_allclose(got_x, x, rtol=R.RTOL, atol=0, err_msg=what)
        np.testing.assert_allclose(got_v, v, rtol=R.RTOL, atol=0, err_msg=what)


@functools.lru_cache(maxsize=None)
def thermalisation_system():
    return R.system(5462, seed=5462, temperature=600.0)


@pytest.mark.parametrize("which", ("restatement", "driver"))
def test_thermalisation(which):
    """600 K to 300 K with friction dt = 50 (c1 = 2e-22: the O step redraws the velocities): the kinetic temperature is within
    5 % of the target after 1, 3 and 25 steps.  Statistical spread sqrt(2 / 3N) = 1.1 %, plus about 1 % from the closing half
    kick; the restatement gave 305.65 K, 307.36 K and 302.68 K."""
    m, x, v = thermalisation_system()
    n = len(m)
    assert abs(2.0 * 0.5 * np.sum(m[:, None] * v * v) / (3 * n * R.KB) - 600.0) < 0.05 * 600.0
    if which == "restatement":
        run = R.Restated(R.force_numpy, m, DT, T, 50.0 / DT, x, v, seed=R.SEED)
        temperature = lambda: run.kinetic_temperature  # noqa: E731
    else:
        run = Langevin(R.torch_force_step(), torch.from_numpy(m), DT, T, 50.0 / DT, torch.from_numpy(x), torch.from_numpy(v),
                       seed=R.SEED)
        temperature = lambda: run.temperature  # noqa: E731
    done = 0
    for upto in (1, 3, 25):
        run.run(upto - done)
        done = upto
        t = temperature()
        print(f"{which}: after {upto} steps {t:.2f} K")
        assert abs(t - T) < 0.05 * T, f"{which}: {t} K after {upto} steps"


def test_reading_does_not_disturb_the_trajectory():
    quiet, _ = make(7)
    read, _ = make(7)
    for _ in range(10):
        quiet.step()
        read.step()
        read.velocities, read.temperature, read.kinetic_energy, read.potential_energy, read.nsteps
    assert torch.equal(quiet.positions, read.positions) and torch.equal(quiet.velocities, read.velocities)


def test_state_dict_round_trip_continues_bit_for_bit():
    whole, _ = make(7)
    whole.run(20)
    first, _ = make(7)
    first.run(10)
    state = first.state_dict()
    assert state["nsteps"] == 10 and state["seed"] == R.SEED and state["friction"] == FRICTION
    assert set(state) == {"positions", "velocities", "nsteps", "timestep", "temperature", "friction", "seed"}
    second, _ = make(7, noise_seed=5)  # (the same atoms somewhere else: everything but the masses must come from the state)
    second.run(3)
    second.set_temperature(1.0)
    second.set_friction(3.0 * FRICTION)
    second.set_timestep(2.0 * DT)
    second.load_state_dict(state)
    second.run(10)
    assert second.nsteps == 20 and second.seed == R.SEED and second.friction == FRICTION
    assert torch.equal(second.positions, whole.positions) and torch.equal(second.velocities, whole.velocities)
    with pytest.raises(ValueError, match="atoms"):
        make(3)[0].load_state_dict(state)
    # the two ensembles do not take each other's states
    m, x, v = (torch.from_numpy(a) for a in R.system(7))
    nh = NoseHoover(R.torch_force_step(), m, DT, T, 0.05, x, v)
    with pytest.raises(ValueError, match="Langevin"):
        second.load_state_dict(nh.state_dict())
    with pytest.raises(ValueError, match="Nose-Hoover"):
        nh.load_state_dict(state)


def test_set_temperature_friction_and_timestep_in_mid_run():
    drv, ref = make(7)
    drv.run(5), ref.run(5)
    drv.set_temperature(900.0)
    ref.temperature = 900.0
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the temperature change")
    drv.set_friction(7.0 * FRICTION)
    ref.friction = 7.0 * FRICTION
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the friction change")
    drv.set_timestep(0.5 * DT)
    ref.dt = 0.5 * DT
    assert drv._c1 == math.exp(-7.0 * FRICTION * 0.5 * DT)
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the time-step change")
    for call, word in ((lambda: drv.set_temperature(-1.0), "temperature"), (lambda: drv.set_friction(-1.0), "friction"),
                       (lambda: drv.set_friction(math.inf), "friction"), (lambda: drv.set_timestep(0.0), "timestep")):
        with pytest.raises(ValueError, match=word):
            call()


def test_argument_refusals_say_which():
    m, x, v = (torch.from_numpy(a) for a in R.system(4))
    step = R.torch_force_step()
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="friction must be non-negative and finite"):
            Langevin(step, m, DT, T, bad, x)
    with pytest.raises(ValueError, match="temperature must be non-negative"):
        Langevin(step, m, DT, -1.0, FRICTION, x)
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError, match="seed must be an integer in"):
            Langevin(step, m, DT, T, FRICTION, x, seed=bad)
    Langevin(step, m, DT, T, FRICTION, x, seed=2 ** 64 - 1)
    with pytest.raises(ValueError, match="mixed devices.*masses on meta"):
        Langevin(step, m.to("meta"), DT, T, FRICTION, x)
    with pytest.raises(ValueError, match="mixed devices.*velocities on meta"):
        Langevin(step, m, DT, T, FRICTION, x, v.to("meta"))
    with pytest.raises(ValueError, match="mixed devices.*forces on meta"):
        Langevin(lambda p: {"forces": p.to("meta"), "total_energy": p.sum()}, m, DT, T, FRICTION, x)
    with pytest.raises(ValueError, match="masses must be positive"):
        Langevin(step, -m, DT, T, FRICTION, x)
    with pytest.raises(ValueError, match="timestep"):
        Langevin(step, m, 0.0, T, FRICTION, x)
    with pytest.raises(ValueError, match="backend='hip' needs device tensors"):
        Langevin(step, m, DT, T, FRICTION, x, backend="hip")
    with pytest.raises(TypeError, match="callable"):
        Langevin(None, m, DT, T, FRICTION, x)


def test_from_atoms_and_write_back():
    m, x, v = R.system(5, seed=4)
    atoms = R.FakeAtoms(["H"] * 5, x, m, v)
    drv = Langevin.from_atoms(atoms, R.torch_force_step(), DT, T, FRICTION, device="cpu", seed=11)
    ref = R.Restated(R.force_numpy, m, DT, T, FRICTION, x, v, seed=11)
    drv.run(3), ref.run(3)
    R.assert_close(drv, ref, "from_atoms")
    drv.write_back(atoms)
    np.testing.assert_allclose(atoms.get_positions(), ref.x, rtol=R.RTOL, atol=R.X_ATOL)
    np.testing.assert_allclose(atoms.get_velocities(), ref.v, rtol=R.RTOL, atol=R.v_atol(T))
    # remove_drift is off by default (the velocities above were taken as they are) and works when asked for
    still = Langevin.from_atoms(R.FakeAtoms(["H"] * 5, x, m, v + 0.3), R.torch_force_step(), DT, T, FRICTION, device="cpu",
                                remove_drift=True)
    p = (m[:, None] * still.velocities.numpy()).sum(0)
    assert np.abs(p).max() < 1e-12 * np.abs(m[:, None] * v).sum()
    model = torch.nn.Linear(1, 1).eval()
    model.type_names = ["H"]
    with pytest.raises(ValueError, match="r_max"):
        Langevin.from_atoms(atoms, model, DT, T, FRICTION, device="cpu")


def test_kernels_are_declared_bound_and_built():
    from nequip_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nequip_amd.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("nqa_md_langevin_step", "nqa_md_noise"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in nequip_amd.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["nqa_md_langevin_step"][1]) == 12 and len(_lib.SIGNATURES["nqa_md_noise"][1]) == 6
    # the record the host writes word by word is the struct of the header, and its size is the one md.hip asserts
    fields = re.search(r"typedef struct nqa_md_langevin_params \{(.*?)\}", header, flags=re.S).group(1)
    names = re.findall(r"\b([a-zA-Z0-9_]+)\s*[,;]", fields)
    assert names == ["c1", "c2", "kT", "seed"]
    assert [md_module._C1, md_module._C2, md_module._KT, md_module._SEED] == list(range(4))
    source = open(os.path.join(ROOT, "nequip_amd", "csrc", "md.hip")).read()
    size = re.search(r"static_assert\(sizeof\(nqa_md_langevin_params\) == (\d+)", source)
    assert size and int(size.group(1)) == 8 * len(names)
    assert re.search(r"static_assert\(sizeof\(nqa_md_state\) == 64", source)  # (the existing record did not grow)
    assert units.kB == R.KB
