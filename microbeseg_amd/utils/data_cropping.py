""" Training crop proposals with optional pre-labelling, on the device.

Reference: ``DataCropWorker`` (src/utils/data_cropping.py: constructor :26-105, ``next_crop`` :138-268, ``inference``
:270-316).  The reference pulls one plane after the other from an OMERO server, takes its statistics with four numpy
passes, cuts up to three crops and sends every crop alone through the network and the post-processing.  Here a frame is
uploaded once, ``mseg_frame_stats`` reduces it in one pass, ``mseg_crops_extract`` cuts its crops with their three
normalisations in one launch (csrc/prepare.hip), and with pre-labelling the crops of up to ``batch_frames`` frames — all
``crop_size`` x ``crop_size`` whatever the frame size — go through ONE network forward and one batched post-processing
call.  The OMERO plumbing is not part of this build: ``crops_local`` is the local route.  DESIGN.md §6i states the rules,
the reference quirks kept and the divergences.
"""
import ctypes as C
import math
import random

import numpy as np
import torch

from .. import _lib
from .qt_shim import QObject, pyqtSignal, pyqtSlot

OOM_MESSAGE = 'RuntimeError during inference (maybe not enough ram/vram?)'


def propose_origins(shape, crop_size, rng):
    """ Crop origins of one frame, the rule of data_cropping.py:157-199 restated: ``None`` for a frame that is skipped
    (an axis shorter than 0.9 * crop_size), else a list of ``(y_start, x_start)`` in the padded frame, one per crop.

    Kept as the reference has them: up to three crops along the longer axis (strictly more than 3 resp. 2 crop sizes);
    the segment length ``c`` from the PADDED extent; the condition ``x_pads > 0 and x_pads > 0`` (a frame padded in y alone
    still draws its column); a frame padded in x gets (0, 0) for every one of its crops; and the order of the draws —
    row first, column second — on ``rng``, a ``random.Random`` (``randint`` bounds inclusive).
    """
    h, w = int(shape[0]), int(shape[1])
    crop_dim = 0 if h > w else 1
    extent = (h, w)[crop_dim]
    if extent > 3 * crop_size:
        n_crops = 3
    elif extent > 2 * crop_size:
        n_crops = 2
    else:
        n_crops = 1
    if 0.9 * crop_size > h or 0.9 * crop_size > w:
        return None
    x_pads, y_pads = max(0, crop_size - w), max(0, crop_size - h)
    ph, pw = h + y_pads, w + x_pads
    extent = (ph, pw)[crop_dim]
    origins = []
    for i in range(n_crops):
        c = extent // n_crops
        if x_pads > 0 and x_pads > 0:
            a, b = 0, 0
        elif crop_dim == 0 and y_pads == 0 and extent > crop_size:
            a = rng.randint(i * c, min(extent - crop_size, (i + 1) * c - crop_size))
            b = rng.randint(0, pw - crop_size)
        elif crop_dim == 1 and x_pads == 0 and extent > crop_size:
            a = rng.randint(0, ph - crop_size)
            b = rng.randint(i * c, min(extent - crop_size, (i + 1) * c - crop_size))
        else:
            a, b = 0, 0
        origins.append((a, b))
    return origins


def stats_from_sums(vmin, vmax, s, q, n):
    """exact integers {min, max, sum v, sum v^2} of n pixels -> (mean, std) in fp64: exact up to the final division and
    square root (np.mean / np.std round log2(n) times on the way)"""
    s, q, n = int(s), int(q), int(n)
    return s / n, math.sqrt(n * q - s * s) / n


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _pix(dtype):
    return 0 if dtype == np.uint8 else 1


def _to_device(a, dev):
    """uint8 / uint16 host array -> device tensor (uint16 bits in int16 storage)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def frame_stats_device(raw):
    """2-D uint8 / uint16-as-int16 device tensor -> Python ints (min, max, sum v, sum v^2)"""
    lib = _lib.load()
    out = torch.empty(4, dtype=torch.int64, device=raw.device)
    _lib.check(lib.mseg_frame_stats(raw.data_ptr(), 0 if raw.dtype == torch.uint8 else 1, raw.numel(), out.data_ptr(),
                                    _stream(raw.device)), "frame_stats")
    return tuple(int(v) for v in out.cpu().numpy().view(np.uint64))


def extract_crops_device(raw, np_dtype, origins, crop_size, pad_value, lo, hi, want=("raw", "show", "u16", "x")):
    """crops of one device frame -> dict of device tensors: raw [K, S, S] (frame dtype), show uint8, u16 (int16 storage),
    x fp32 [K, 1, S, S]; only the outputs named in ``want`` are produced"""
    lib = _lib.load()
    dev = raw.device
    K, S = len(origins), int(crop_size)
    H, W = raw.shape
    org = torch.tensor(np.asarray(origins, np.int32).reshape(K, 2), dtype=torch.int32, device=dev)
    out = {}
    if "raw" in want:
        out["raw"] = torch.empty((K, S, S), dtype=raw.dtype, device=dev)
    if "show" in want:
        out["show"] = torch.empty((K, S, S), dtype=torch.uint8, device=dev)
    if "u16" in want:
        out["u16"] = torch.empty((K, S, S), dtype=torch.int16, device=dev)
    if "x" in want:
        out["x"] = torch.empty((K, 1, S, S), dtype=torch.float32, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None      # noqa: E731
    _lib.check(lib.mseg_crops_extract(raw.data_ptr(), _pix(np_dtype), H, W, K, org.data_ptr(), S, int(pad_value), int(lo),
                                      int(hi), ptr("raw"), ptr("show"), ptr("u16"), ptr("x"), _stream(dev)),
               "crops_extract")
    return out


def _host(t):
    """device tensor -> host array (int16 storage viewed as the uint16 it holds)"""
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


class DataCropWorker(QObject):
    """ Worker class for training crop creation (reference data_cropping.py:19-330: same constructor, signals and slots).
    The OMERO route (``connect``, ``next_crop``, ``get_crop``) is not part of this build and raises like
    ``AnalysisWorker.analyze_data``; ``crops_local`` is the local route and ``inference`` keeps the reference's surface. """
    finished = pyqtSignal()  # Signal when cropping is finished
    text_output = pyqtSignal(str)  # Signal for possible exceptions, e.g., too small crops
    crops = pyqtSignal(object)  # Signal for sending the crops
    stop_creation = False
    # same meaning as InferWorker.precision / InferWorker.prediction_hook (the hook sees every crop's (1, C, S, S) prediction,
    # in crop order)
    precision = "fp32"
    prediction_hook = None

    def __init__(self, img_list=None, crop_size=256, trainset_id=None, train_path=None, omero_username=None,
                 omero_password=None, omero_host=None, omero_port=None, group_id=None, pre_labeling=False, model=None,
                 device=None, num_gpus=None, ths=None):
        super().__init__()
        self.img_list = img_list
        self.crop_size = crop_size
        self.trainset_id = trainset_id
        self.train_path = train_path
        self.img_idx = 0
        self.crop = None
        self.pre_labeling = pre_labeling
        self.omero_username = omero_username
        self.omero_password = omero_password
        self.omero_host = omero_host
        self.omero_port = omero_port
        self.group_id = group_id
        self.conn = None
        self.device = torch.device(device) if device is not None else None
        self.net, self.model_settings, self.ths = None, None, None
        self._infer = None
        if self.pre_labeling:
            self._load_model(model, ths)

    def _load_model(self, model, ths):
        from ..inference.infer import InferWorker
        if self.device is None:
            self.device = torch.device("cuda:0")
        self._infer = InferWorker(model=str(model), device=self.device, ths=tuple(ths) if ths is not None else (0.10, 0.45))
        self._infer.text_output.connect(self.text_output.emit)
        self.net, self.model_settings = self._infer.net, self._infer.model_settings
        self.ths = list(ths) if (ths is not None and self.model_settings['label_type'] == 'distance') else \
            (self._infer.ths if self.model_settings['label_type'] == 'distance' else None)

    # -- OMERO route: not part of this build -----------------------------------------------------------------------------
    def _no_omero(self, name):
        raise RuntimeError(f"DataCropWorker.{name} needs the OMERO stack (omero-py), which is outside the MI355X hot "
                           "path; use DataCropWorker.crops_local() or prepare_script.py crops")

    def connect(self):
        self._no_omero("connect")

    def disconnect(self):
        self.conn = None

    def get_crop(self):
        self._no_omero("get_crop")

    def next_crop(self):
        self._no_omero("next_crop")

    # -- the reference's one-crop surface ---------------------------------------------------------------------------------
    def inference(self, crop, min_val, max_val):
        """ Prediction of ONE un-padded crop for pre-labelling (data_cropping.py:270-316): normalisation with the frame's
        minimum / maximum, network forward, post-processing, all on the device.  An out-of-memory or shape RuntimeError of
        the forward gives a zero mask and the reference's message.

        :return: instance mask, np.uint16, shape of the crop
        """
        from ..inference.infer import normalize_host
        worker = self._require_model()
        crop = np.asarray(crop)
        img_batch = normalize_host(crop, min_val, max_val)
        x = torch.from_numpy(np.ascontiguousarray(img_batch[None, None, :, :])).to(torch.float)
        with torch.cuda.device(self.device), torch.no_grad():
            masks = self._predict(worker, x.to(self.device), shape_errors_too=True)
        return _host(masks)[0]

    def _require_model(self):
        if self._infer is None:
            raise RuntimeError("pre-labelling needs a model: DataCropWorker(..., pre_labeling=True, model=<path>)")
        self._infer.precision = self.precision
        if self.ths is not None:                     # (distance models: the thresholds its post-processing step reads)
            self._infer.ths = self.ths
        self._infer.net.eval()
        return self._infer

    @staticmethod
    def _is_shape_error(err):
        return isinstance(err, RuntimeError) and "not divisible" in str(err)

    def _predict(self, worker, x, cap=None, shape_errors_too=False):
        """(n, 1, S, S) network input on the device -> int16-storage uint16 masks (n, S, S) on the device.  One forward for
        all n (at most ``cap[0]`` per forward once an out-of-memory halved the group: InferWorker._forward_group), the
        hook per crop and one InferWorker._postprocess_group per forward.  ``worker`` comes from ``_require_model``, which
        has set its precision and, for distance models, its thresholds to this object's: the post-processing step reads
        ``worker.ths``, not ``self.ths``."""
        from ..inference.infer import hook_per_frame
        n, _, S, _ = x.shape
        boundary = self.model_settings['label_type'] != 'distance'
        masks = torch.zeros((n, S, S), dtype=torch.int16, device=x.device)
        cap = cap if cap is not None else [n]
        i = 0
        while i < n:
            m = min(max(1, cap[0]), n - i)
            try:
                chunks, size = worker._forward_group(x[i:i + m])
            except RuntimeError as err:
                if not (shape_errors_too and self._is_shape_error(err)):
                    raise
                self.text_output.emit(OOM_MESSAGE)
                chunks, size = [(0, m, None)], cap[0]
            cap[0] = min(cap[0], size)
            for c0, cm, pred in chunks:
                if pred is None:                                  # zero masks, message already sent
                    continue
                if self.prediction_hook is not None:
                    pred = hook_per_frame(self.prediction_hook, pred)
                if boundary:
                    logits = pred.contiguous()
                    pred = (worker._softmax_hwc(logits[j:j + 1], (0, 0)) for j in range(cm))
                else:
                    pred = (pred[0][:, 0], pred[1][:, 0])
                worker._postprocess_group(pred, masks[i + c0:i + c0 + cm], (0, 0))
            i += m
        return masks

    # -- ROIs and overlays of a group of crops ------------------------------------------------------------------------------
    def _rois_and_overlays(self, masks, shows):
        """masks int16 (n, S, S), shows uint8 (n, S, S) on the device -> (list of n ROI string lists, roi_show uint8
        (n, S, S, 3) host): polygons per crop in the order of InferWorker.polygon_rois, all outlines in one
        mseg_roi_outline launch, all overlays in one mseg_crops_overlay launch"""
        from .hull_polygon import label_polygons, points_string
        lib = _lib.load()
        dev = masks.device
        n, S, _ = masks.shape
        rois, rc, lens, frames = [], [], [], []
        for k in range(n):
            strings = []
            for polygons in label_polygons(masks[k]).values():
                for polygon in polygons:
                    strings.append(points_string(polygon))
                    rc.append(polygon.T.astype(np.int32))
                    lens.append(polygon.shape[1])
                    frames.append(k)
            rois.append(strings)
        outl = torch.zeros((n, S, S), dtype=torch.uint8, device=dev)
        if lens:
            voff = np.zeros(len(lens) + 1, np.int64)
            np.cumsum(lens, out=voff[1:])
            rc_d = torch.from_numpy(np.ascontiguousarray(np.concatenate(rc, 0))).to(dev)
            voff_d = torch.from_numpy(voff).to(dev)
            fr_d = torch.from_numpy(np.asarray(frames, np.int32)).to(dev)
            _lib.check(lib.mseg_roi_outline(rc_d.data_ptr(), voff_d.data_ptr(), fr_d.data_ptr(), len(lens), int(voff[-1]),
                                            n, S, S, outl.data_ptr(), _stream(dev)), "roi_outline")
        rgb = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        _lib.check(lib.mseg_crops_overlay(shows.data_ptr(), outl.data_ptr(), rgb.data_ptr(), n, S, _stream(dev)),
                   "crops_overlay")
        return rois, rgb.cpu().numpy()

    # -- local route ------------------------------------------------------------------------------------------------------
    def crops_local(self, frames, crop_size=None, pre_labeling=None, model=None, ths=None, device=None, rng=None,
                    batch_frames=8, text_output=None):
        """ Crop proposals for an iterable of 2-D host frames of any (different) sizes: the list, per accepted frame, of the
        reference's list of crop dicts (data_cropping.py:247-264 without the OMERO ids): ``crop_size``, ``min_frame``,
        ``max_frame``, ``mean_frame``, ``std_frame``, ``pre_labeled``, ``x_start``, ``y_start`` (strings as the reference
        formats them), ``frame`` (here: the index of the frame in ``frames``), ``img``, ``img_show``, ``roi`` (list of "x,y x,y " strings) and ``roi_show`` (None without
        pre-labelling), with pre-labelling also ``mask`` [extension]: the predicted uint16 instance mask the ROIs trace.  Frames that are too small are skipped like in the reference; constant frames are skipped with a
        message (the reference divides by zero there).  ``rng``: a ``random.Random`` (default: a fresh one). """
        S = int(self.crop_size if crop_size is None else crop_size)
        pre = self.pre_labeling if pre_labeling is None else bool(pre_labeling)
        say = text_output if text_output is not None else self.text_output.emit
        if device is not None:
            self.device = torch.device(device)
        if self.device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("No MI355X visible: crops are cut on the device (there is no CPU path)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        if pre and (model is not None or self._infer is None):
            if model is None:
                raise RuntimeError("pre-labelling needs a model")
            self._load_model(model, ths)
        elif pre and ths is not None and self.model_settings['label_type'] == 'distance':
            self.ths = list(ths)
        rng = rng if rng is not None else random.Random()
        worker = self._require_model() if pre else None
        result, group, cap = [], [], [1 << 30]
        dev = self.device

        def flush():
            if not group:
                return
            x = torch.cat([g["x"] for g in group], dim=0)
            shows = torch.cat([g["show"] for g in group], dim=0)
            masks = self._predict(worker, x, cap)
            rois, rgb = self._rois_and_overlays(masks, shows)
            masks_h = _host(masks)
            k = 0
            for g in group:
                for d in g["dicts"]:
                    d['roi'], d['roi_show'], d['mask'] = rois[k], rgb[k], masks_h[k]
                    k += 1
                result.append(g["dicts"])
            group.clear()

        with torch.cuda.device(dev), torch.no_grad():
            for index, frame in enumerate(frames):
                if self.stop_creation:
                    break
                frame = np.asarray(frame)
                if frame.ndim != 2:
                    raise RuntimeError("crops_local: 2-D frames expected")
                on_device = frame.dtype in (np.uint8, np.uint16)
                if on_device:
                    raw = _to_device(frame, dev)
                    vmin, vmax, s, q = frame_stats_device(raw)
                    mean, std = stats_from_sums(vmin, vmax, s, q, frame.size)
                    vmin, vmax = frame.dtype.type(vmin), frame.dtype.type(vmax)
                else:
                    vmin, vmax, mean, std = np.min(frame), np.max(frame), np.mean(frame), np.std(frame)
                origins = propose_origins(frame.shape, S, rng)
                if origins is None:
                    continue
                if vmax == vmin:
                    say(f"  frame {index}: constant frame --> skip")
                    continue
                if on_device:
                    out = extract_crops_device(raw, frame.dtype, origins, S, vmin, vmin, vmax,
                                               want=("raw", "show", "x") if pre else ("raw", "show"))
                    imgs, shows_h = _host(out["raw"]), out["show"].cpu().numpy()
                else:
                    out = self._extract_host(frame, origins, S, vmin, vmax, pre, dev)
                    imgs, shows_h = out["raw_host"], out["show_host"]
                dicts = []
                for k, (a, b) in enumerate(origins):
                    dicts.append({'frame': index, 'crop_size': str(S),
                                  'max_frame': str(vmax), 'mean_frame': str(np.float64(mean)), 'min_frame': str(vmin),
                                  'std_frame': str(np.float64(std)), 'pre_labeled': str(False),
                                  'x_start': str(b), 'y_start': str(a),
                                  'img': imgs[k], 'img_show': shows_h[k],
                                  'roi': None, 'roi_show': None})
                if not pre:
                    result.append(dicts)
                    continue
                group.append({"x": out["x"], "show": out["show"], "dicts": dicts})
                if len(group) >= max(1, int(batch_frames)):
                    flush()
            flush()
        return result

    @staticmethod
    def _extract_host(frame, origins, S, vmin, vmax, pre, dev):
        """frames of other dtypes than uint8 / uint16: the reference's formulas on the host (like InferWorker._group_input)"""
        from ..inference.infer import normalize_host
        y_pads, x_pads = max(0, S - frame.shape[0]), max(0, S - frame.shape[1])
        img = np.pad(frame, ((0, y_pads), (0, x_pads)), mode='constant', constant_values=vmin)
        raws, shows, xs = [], [], []
        for a, b in origins:
            crop = img[a:a + S, b:b + S]
            raws.append(crop)
            shows.append((255 * (crop.astype(np.float32) - vmin) / (vmax - vmin)).astype(np.uint8))
            xs.append(normalize_host(crop, vmin, vmax))
        out = {"raw_host": np.stack(raws), "show_host": np.stack(shows)}
        out["show"] = torch.from_numpy(out["show_host"]).to(dev)
        if pre:
            out["x"] = torch.from_numpy(np.ascontiguousarray(np.stack(xs)[:, None].astype(np.float32))).to(dev)
        return out

    @pyqtSlot()
    def crop_creation_finished(self):
        """ Send finished signal """
        self.disconnect()
        self.finished.emit()

    @pyqtSlot()
    def stop_crop_process(self):
        """ Set internal stop state to True """
        self.stop_creation = True


def crops_local(frames, crop_size, pre_labeling=False, model=None, ths=None, device=None, rng=None, batch_frames=8,
                text_output=print):
    """ ``DataCropWorker.crops_local`` without building the worker first: see there.  Messages (skipped frames, a forward
    that ran out of memory) go to ``text_output``. """
    worker = DataCropWorker(crop_size=crop_size, device=device)
    worker.text_output.connect(text_output)
    return worker.crops_local(frames, crop_size, pre_labeling=pre_labeling, model=model, ths=ths, rng=rng,
                              batch_frames=batch_frames)
