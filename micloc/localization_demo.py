"""Drop-in alias: `micloc.localization_demo` -> haghighatshoarmuir2024_amd.localization_demo (hardware-free Demo of the complex Beamformer)."""
from haghighatshoarmuir2024_amd.localization_demo import Demo  # noqa: F401
