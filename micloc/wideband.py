"""Drop-in alias: `micloc.wideband` -> haghighatshoarmuir2024_amd.wideband (batched wideband localisation, SNN and complex)."""
from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer  # noqa: F401
