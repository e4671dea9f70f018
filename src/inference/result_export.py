from microbeseg_amd.inference.result_export import ResultExportWorker, overlay, export_local  # noqa: F401
