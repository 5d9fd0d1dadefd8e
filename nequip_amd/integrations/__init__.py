from .md import Langevin, NoseHoover, VelocityVerlet, langevin_noise, maxwell_boltzmann_velocities, units
from .relax import FIRE

__all__ = ["FIRE", "Langevin", "NoseHoover", "VelocityVerlet", "langevin_noise", "maxwell_boltzmann_velocities", "units"]
