from microbeseg_amd.inference.analysis import AnalysisWorker, make_coordinates, rois_to_masks, analyze_masks, analyze_local  # noqa: F401
