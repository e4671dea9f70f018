from microbeseg_amd.utils.data_cropping import DataCropWorker, propose_origins, crops_local  # noqa: F401
