from .md import Langevin, LangevinNPT, NoseHoover, VelocityVerlet, langevin_noise, maxwell_boltzmann_velocities, units
from .md_batched import BatchedLangevin, BatchedLangevinNPT
from .relax import FIRE, CellFIRE

__all__ = ["BatchedLangevin", "BatchedLangevinNPT", "CellFIRE", "FIRE", "Langevin", "LangevinNPT", "NoseHoover", "VelocityVerlet",
           "langevin_noise", "maxwell_boltzmann_velocities", "units"]
