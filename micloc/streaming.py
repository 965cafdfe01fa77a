"""Drop-in alias: `micloc.streaming` -> haghighatshoarmuir2024_amd.streaming (a recording delivered tile by tile, one band or wideband)."""
from haghighatshoarmuir2024_amd.streaming import (  # noqa: F401
    ComplexStreamingLocalizer,
    StreamingLocalizer,
    WidebandComplexStreamingLocalizer,
    WidebandStreamingLocalizer,
)
