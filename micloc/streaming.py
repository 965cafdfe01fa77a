"""Drop-in alias: `micloc.streaming` -> haghighatshoarmuir2024_amd.streaming (a recording delivered tile by tile, one band or wideband)."""
from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer, StreamingLocalizer, WidebandStreamingLocalizer  # noqa: F401
