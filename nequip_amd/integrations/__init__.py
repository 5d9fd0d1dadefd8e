from .md import NoseHoover, VelocityVerlet, maxwell_boltzmann_velocities, units

__all__ = ["NoseHoover", "VelocityVerlet", "maxwell_boltzmann_velocities", "units"]
