"""Drop-in alias: `micloc.wideband` -> haghighatshoarmuir2024_amd.wideband (batched wideband SNN localisation)."""
from haghighatshoarmuir2024_amd.wideband import WidebandSNNLocalizer  # noqa: F401
