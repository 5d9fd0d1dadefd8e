from .md import Langevin, LangevinNPT, NoseHoover, VelocityVerlet, langevin_noise, maxwell_boltzmann_velocities, units
from .relax import FIRE, CellFIRE

__all__ = ["CellFIRE", "FIRE", "Langevin", "LangevinNPT", "NoseHoover", "VelocityVerlet", "langevin_noise", "maxwell_boltzmann_velocities",
           "units"]
