"""Drop-in `micloc` package: the reference's import paths (micloc.snn_beamformer, micloc.beamformer,
micloc.spike_encoder, micloc.array_geometry, micloc.utils, micloc.filterbank, micloc.music_beamformer, micloc.localization_demo_snn, micloc.localization_demo,
micloc.localization_demo_MUSIC) backed by the MI355X
implementation in haghighatshoarmuir2024_amd, and the forms the reference lacks (micloc.wideband, micloc.streaming)."""
