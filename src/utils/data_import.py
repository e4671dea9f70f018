from microbeseg_amd.utils.data_import import DataImportWorker  # noqa: F401
