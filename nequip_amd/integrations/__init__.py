from .md import Langevin, NoseHoover, VelocityVerlet, langevin_noise, maxwell_boltzmann_velocities, units
from .relax import FIRE, CellFIRE

__all__ = ["CellFIRE", "FIRE", "Langevin", "NoseHoover", "VelocityVerlet", "langevin_noise", "maxwell_boltzmann_velocities",
           "units"]
