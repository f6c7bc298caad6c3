"""detzero_track - the package name of the reference's tracking stage (tracking/detzero_track), re-exporting the MI355X mirrors:
``models`` (detzero_amd.track_models: the tracker on the device table), ``datasets`` (detzero_amd.track_models, in-process loader)
and ``utils`` (detzero_amd.track_adapter)."""
