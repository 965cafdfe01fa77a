"""Drop-in alias: `micloc.music_beamformer` -> haghighatshoarmuir2024_amd.music_beamformer (MI355X implementation)."""
from haghighatshoarmuir2024_amd.music_beamformer import *  # noqa: F401,F403
from haghighatshoarmuir2024_amd import music_beamformer as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
