from .md import Langevin, NoseHoover, VelocityVerlet, langevin_noise, maxwell_boltzmann_velocities, units

__all__ = ["Langevin", "NoseHoover", "VelocityVerlet", "langevin_noise", "maxwell_boltzmann_velocities", "units"]
