"""Drop-in alias: `micloc.localization_demo_MUSIC` -> haghighatshoarmuir2024_amd.localization_demo_MUSIC (hardware-free Demo of MUSIC)."""
from haghighatshoarmuir2024_amd.localization_demo_MUSIC import Demo  # noqa: F401
