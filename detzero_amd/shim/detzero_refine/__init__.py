"""detzero_refine - the package name of the reference's refining stage (refining/detzero_refine), re-exporting the MI355X
mirrors: ``models`` (detzero_amd.refine_models) and ``datasets`` (detzero_amd.refine_dataset, test mode)."""
