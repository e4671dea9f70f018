"""A training set that is read once and stays in HBM (``TrainWorker.resident``).

The loader route (``TrainingDataset`` + ``DataLoader`` + ``_Feeder``) reads three TIFF files per crop in every epoch, collates
and pins them in worker processes and uploads them.  A training set is small beside 288 GB of HBM (1000 distance crops of
320^2: 0.2 GB uint16 + 2 x 0.4 GB fp32), so this route reads every crop once, keeps one tensor per plane and split on the
device, and makes a step's batch with one ``mseg_set_gather`` launch per plane:

  ``load_host``        the host stage (no GPU needed): all crops of 'train' and 'val' through ``utils.tiffio`` into one
                       contiguous array per plane and split, by the file-name rule of ``TrainingDataset``
  ``resident_fits``    the budget rule as a pure function
  ``ResidentSet``      the uploaded planes; ``batch(split, indices, training)`` returns what ``_Feeder.__call__`` works on
                       after its ``.to(device)``: same shapes and values; where the train phase feeds ``DeviceAugment`` the
                       image stays uint16 (instead of int32) and a boundary label is fp32 (instead of int64), the types it
                       converts to anyway
  ``ResidentBatches``  per phase, what the ``DataLoader`` is on the loader route: an iterable over the plan's steps that
                       consumes torch's default generator exactly like ``iter(DataLoader(...))``
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib
from ..utils import tiffio as tiff

SPLITS = ('train', 'val')
DEFAULT_MAX_BYTES = 8 << 30     # about 8000 distance crops of 320^2: 8x the top row of get_max_epochs' table, 3 % of HBM
MAX_THREADS = 16                # never sized from cpu_count: a shared machine shows all its CPUs

# label type -> planes in batch order: (name, file prefix, dtype in HBM)
PLANES = {
    'distance': (('img', 'img', np.uint16), ('border_label', 'neighbor_dist', np.float32),
                 ('cell_label', 'cell_dist', np.float32)),
    'boundary': (('img', 'img', np.uint16), ('label', 'boundary', np.uint8)),
}


class ResidentUnavailable(Exception):
    """The set cannot be held on the device; ``TrainWorker`` falls back to the loader route and says why."""


class MixedCropShapes(ResidentUnavailable):
    """The crops of one split differ in shape: they do not form one [n][H][W] plane."""


def resident_fits(set_bytes, max_bytes, free_bytes):
    """Budget rule: resident if the set needs at most ``max_bytes`` and at most a quarter of the free device memory."""
    return set_bytes <= max_bytes and 4 * set_bytes <= free_bytes


def _host_array(shape, dtype, pin):
    if pin:
        try:
            t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), pin_memory=True)
            return t.numpy()
        except (RuntimeError, TypeError):   # no device to pin for, or a dtype this torch cannot pin: pageable memory
            pass
    return np.empty(shape, dtype=dtype)


def _as_plane_dtype(a, name, dtype, file):
    if a.ndim != 2:
        raise ResidentUnavailable('{} is not a 2D image'.format(file.name))
    if name == 'img' and a.dtype not in (np.uint8, np.uint16):
        raise ResidentUnavailable('{} is {}, not uint8 / uint16'.format(file.name, a.dtype))
    return a.astype(dtype, copy=False)


def load_host(root_dir, label_type, threads=8, pin=False):
    """-> {split: {plane name: ndarray [n][H][W]}}: every crop of ``root_dir/{train,val}`` read once."""
    if label_type not in PLANES:
        raise Exception('Unknown label type')
    threads = max(1, min(int(threads), MAX_THREADS))
    out = {}
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for split in SPLITS:
            ids = sorted((root_dir / split).glob('img*.tif'))         # TrainingDataset's list and order
            if not ids:
                raise ResidentUnavailable('no crops in {}'.format(split))
            planes = {}
            for name, prefix, dtype in PLANES[label_type]:
                files = [f.parent / (prefix + f.name.split('img')[-1]) for f in ids]
                first = _as_plane_dtype(tiff.imread(str(files[0])), name, dtype, files[0])
                arr = _host_array((len(files),) + first.shape, dtype, pin)
                arr[0] = first

                def read(i, arr=arr, files=files, name=name, dtype=dtype):
                    a = _as_plane_dtype(tiff.imread(str(files[i])), name, dtype, files[i])
                    if a.shape != arr.shape[1:]:
                        raise MixedCropShapes('{} is {}x{}, {} is {}x{}'.format(
                            files[i].name, a.shape[0], a.shape[1], files[0].name, *arr.shape[1:]))
                    arr[i] = a
                list(pool.map(read, range(1, len(files))))
                planes[name] = arr
            shapes = {a.shape for a in planes.values()}
            if len(shapes) != 1:
                raise MixedCropShapes('image and label planes of {} differ in shape'.format(split))
            out[split] = planes
    return out


def host_bytes(host):
    return int(sum(a.nbytes for planes in host.values() for a in planes.values()))


def _is_oom(err):
    text = str(err).lower()
    return 'out of memory' in text or 'hiperroroutofmemory' in text


_SRC = {np.dtype(np.uint8): _lib.PIX_U8, np.dtype(np.uint16): _lib.PIX_U16, np.dtype(np.float32): _lib.PIX_F32}
_DST = {_lib.GATHER_RAW: None, _lib.GATHER_F32: torch.float32, _lib.GATHER_NORM: torch.float32,
        _lib.GATHER_I64: torch.int64}


def set_gather(src, idx, mode, lo=0.0, hi=1.0):
    """``mseg_set_gather`` on torch tensors: src [n][H][W] (uint8 / uint16 / int16 holding uint16 bits / fp32) and idx
    int32 [N] on one device -> [N][H][W] of the type ``mode`` names (``_lib.GATHER_*``)."""
    dtype = {torch.int16: np.dtype(np.uint16)}.get(src.dtype) or np.dtype(str(src.dtype).split('.')[-1])
    if dtype not in _SRC or mode not in _DST or not src.is_contiguous() or idx.dtype != torch.int32:
        raise ValueError('set_gather: unsupported source {} / mode {}'.format(src.dtype, mode))
    n, hw = src.shape[0], int(np.prod(src.shape[1:]))
    out_dtype = _DST[mode] or (torch.uint16 if dtype == np.uint16 else src.dtype)
    out = torch.empty((idx.numel(),) + tuple(src.shape[1:]), dtype=out_dtype, device=src.device)
    idx = idx.contiguous()
    _lib.check(_lib.load().mseg_set_gather(src.data_ptr(), _SRC[dtype], n, hw, idx.data_ptr(), idx.numel(), out.data_ptr(),
                                           mode, float(lo), float(hi), torch.cuda.current_stream(src.device).cuda_stream),
               'set_gather')
    return out


class ResidentSet:
    """The planes of a training set on the device.  ``raw_train``: the train phase hands un-normalised crops to
    ``DeviceAugment`` (``RawToTensor`` on the loader route); otherwise both phases are ``ToTensor``."""

    def __init__(self, host, label_type, device, min_value, max_value, raw_train, gather=set_gather):
        self.label_type, self.device = label_type, torch.device(device)
        self.min_value, self.max_value, self.raw_train = float(min_value), float(max_value), bool(raw_train)
        self.names = tuple(name for name, _, _ in PLANES[label_type])
        self.sizes = {split: len(host[split]['img']) for split in SPLITS}
        self.nbytes = host_bytes(host)
        self._gather = gather
        self.planes = {}
        try:
            for split in SPLITS:
                self.planes[split] = {name: torch.from_numpy(host[split][name]).to(self.device) for name in self.names}
        except RuntimeError as err:
            self.planes = {}
            if _is_oom(err):
                raise ResidentUnavailable('the upload ran out of device memory') from None
            raise

    def release(self):
        self.planes = {}

    def __len__(self):
        return self.sizes['train'] + self.sizes['val']

    def batch(self, split, indices, training):
        """(image batch, label batches...) of the crops ``indices`` of ``split``, as ``default_collate`` of the
        ``TrainingDataset`` items moved to the device."""
        indices = [int(i) for i in indices]
        n = self.sizes[split]
        for i in indices:                                   # on the host, before any launch
            if not 0 <= i < n:
                raise IndexError('crop index {} out of range for {} crops of {}'.format(i, n, split))
        raw = bool(training) and self.raw_train
        planes = self.planes[split]
        idx = torch.tensor(indices, dtype=torch.int32).to(self.device)
        if raw:
            img = self._gather(planes['img'], idx, _lib.GATHER_RAW)
        else:
            img = self._gather(planes['img'], idx, _lib.GATHER_NORM, self.min_value, self.max_value)
        img = img.unsqueeze(1)
        if self.label_type == 'distance':
            return (img,) + tuple(self._gather(planes[k], idx, _lib.GATHER_RAW).unsqueeze(1) for k in self.names[1:])
        return img, self._gather(planes['label'], idx, _lib.GATHER_F32 if raw else _lib.GATHER_I64)


class ResidentBatches:
    """One phase's batches: the ``DataLoader(dataset, batch_sampler=plan)`` of the resident route.  ``iter()`` takes the one
    draw from torch's default generator that a ``DataLoader`` iterator takes for its base seed, so a seeded run sees the
    same permutations on either route; Python's ``random`` and ``np.random`` (``DeviceAugment``'s sources) stay untouched."""

    def __init__(self, rset, split, plan, training):
        self.rset, self.split, self.plan, self.training = rset, split, plan, training

    def __len__(self):
        return len(self.plan)

    def __iter__(self):
        torch.empty((), dtype=torch.int64).random_()
        return (self.rset.batch(self.split, indices, self.training) for indices in list(self.plan))
