"""Inference driver of the hot path: per frame normalise -> U-Net forward (eval) -> un-pad -> post-processing.

Mirror of ``InferWorker`` in ``src/inference/infer.py`` (reference: constructor :30-111, ``start_inference`` :113-326,
``inference`` :328-376) and of the frame loop of ``infer_script_local.py`` (:118-161).  The OMERO plumbing of
``start_inference`` (login, plane download, ROI upload) is outside the hot path; what is
kept is the per-frame contract — ``inference(img, min_val, max_val, pads)`` with an already padded frame, returning the
``np.uint16`` instance mask of the un-padded frame — plus ``infer_stack`` for local [T, H, W] stacks.
On the MI355X path the frame stays in HBM between the network and the watershed; only the uint16 mask returns.
"""
import itertools
import json
from pathlib import Path

import numpy as np
import torch

from .. import _lib, engine
from ..utils.qt_shim import QObject, pyqtSignal, pyqtSlot
from ..utils.unets import build_unet, get_weights
from ..utils.utils import zero_pad_model_input
from . import postprocessing as pp


def is_out_of_memory(err):
    """The reference turns EVERY RuntimeError of ``self.net(img_batch)`` into an all-zero mask (infer.py:351-356: "maybe
    not enough ram/vram?").  Here only a real allocation failure of the network forward gets that treatment; a kernel
    launch error of libmseg_hip, an asynchronous HIP fault or a shape bug propagates instead of silently writing empty
    segmentations."""
    msg = str(err).lower()
    return isinstance(err, (RuntimeError, MemoryError)) and (
        "out of memory" in msg or "hiperroroutofmemory" in msg or "hip error: out of memory" in msg)


FRAME_BATCH_PIXELS = 2048 * 2048     # pixels of one group of frames (see frame_batch_for)
FRAME_BATCH_AUTO = 64


def frame_batch_for(Hp, Wp, requested):
    """Frames of padded size Hp x Wp that go through the network and the post-processing as ONE group:
    ``max(1, min(requested, 2048 * 2048 // (Hp * Wp)))``; ``requested = 0`` means auto, i.e. ``min(64, ...)``.

    Both constants are choices, not measurements: 2048^2 is the largest whole-frame size whose memory this project has
    exercised, and a group of that many pixels has level-0 activations of the size of one such frame; 64 is the group
    that fills this budget at 256^2.  Pure host arithmetic."""
    cap = FRAME_BATCH_PIXELS // (int(Hp) * int(Wp))
    req = int(requested)
    if req <= 0:
        req = FRAME_BATCH_AUTO
    return max(1, min(req, cap))


def normalize_host(frame, min_val, max_val):
    """2 * (f32(frame) - min) / (max - min) - 1 on the host, same operation order and scalar types as infer.py:346-348
    (``min_val`` / ``max_val``: numpy scalars of the frame's dtype); the device normalisation equals it bit for bit"""
    return 2 * (frame.astype(np.float32) - min_val) / (max_val - min_val) - 1


def hook_per_frame(hook, pred):
    """``hook`` once per frame, in frame order, on that frame's (1, C, Hp, Wp) slice of a group's padded prediction
    (boundary models: logits (n, 3, Hp, Wp); distance models: (border, cell), each (n, 1, Hp, Wp)), concatenated again"""
    if isinstance(pred, torch.Tensor):
        return torch.cat([hook(pred[i:i + 1]) for i in range(pred.shape[0])], dim=0)
    hooked = [hook((pred[0][i:i + 1], pred[1][i:i + 1])) for i in range(pred[0].shape[0])]
    return torch.cat([h[0] for h in hooked], dim=0), torch.cat([h[1] for h in hooked], dim=0)


def load_model(model, device):
    """``model``: path of the checkpoint without/with suffix; reads ``<model>.json`` (architecture, label_type) and
    ``<model>.pth`` (state dict), like infer.py:83-84,119-131.  Returns (net in eval mode, model_settings)."""
    model = Path(model)
    base = model.parent / model.stem
    if not base.with_suffix('.pth').is_file():
        raise Exception(f'{base.with_suffix(".pth")} not found!')
    if not base.with_suffix('.json').is_file():
        raise Exception(f'{base.with_suffix(".json")} not found!')
    with open(base.with_suffix('.json')) as f:
        settings = json.load(f)
    arch = settings['architecture']
    net = build_unet(unet_type=arch[0], act_fun=arch[2], pool_method=arch[1], normalization=arch[3], device=device,
                     num_gpus=1, ch_in=1, ch_out=1 if settings['label_type'] == 'distance' else 3, filters=arch[4])
    net = get_weights(net=net, weights=str(base.with_suffix('.pth')), num_gpus=1, device=device)
    net.eval()
    return net, settings


class InferWorker(QObject):
    """ Worker class for inference """
    finished = pyqtSignal()
    progress = pyqtSignal(int)
    text_output = pyqtSignal(str)
    stop_inference = False
    # [extension] "bf16": the network forward runs with bf16 matrix-core inputs (fp32 accumulate / storage),
    # ~3x faster; predictions differ from the fp32 reference arithmetic in the third digit, so masks are no longer
    # guaranteed bit-identical to the reference's — opt-in only, the default is the reference's fp32
    precision = "fp32"
    # [extension] edge length of the tiles of sliding-window inference (``sliding_window=True``; inference/tiling.py)
    tile_size = 2048
    # [measurement hook, None in production] callable(prediction) -> prediction, applied to the network's output before the
    # post-processing.  bench.py uses it to hand the watershed realistic distance maps: an UNTRAINED network (there are no
    # checkpoints offline) predicts one confluent blob, whose flood is a single sequential component.
    prediction_hook = None
    BOUNDARY_BATCH = 8      # infer_stack, boundary method: frames whose floods share one launch (1..8)
    # [extension] infer_stack: frames per group (one upload, one network forward at batch n, one batched post-processing
    # call per group; frame_batch_for caps it by the frame size).  1 = frame by frame (the default: that path is untouched),
    # 0 = auto.  Made for stacks of small frames (128^2 .. 512^2), where a frame's kernels are too short to fill the GPU.
    frame_batch = 1
    # [extension] infer_stack: every uint8 / uint16 frame is contrast-enhanced on the device before its min / max
    # (utils/clahe.py: the library-exact CLAHE of the reference's ContrastEnhancement) and goes on as a uint16 frame
    apply_clahe = False
    # [extension] cell_table: links between frames that share fewer pixels are dropped (inference/cells.py)
    min_overlap = 1
    # [extension] cell_table: None = link at the same (y, x); R = 0 .. 128: estimate the stage drift of every frame pair
    # within +-R pixels on the device and link under it (inference/cells.py)
    drift = None
    # [extension] cell_table: None = one shift per frame pair; r = 0 .. 32 (needs drift): every flow_tile x flow_tile tile
    # (64, 128 or 256 px) of a frame gets its own shift within +-r pixels of the pair's drift, found on the device, and the
    # cells are linked under that field (inference/cells.py)
    flow = None
    flow_tile = 64
    # [extension] cell_table: None = a cell that is missed in a frame starts a new track; G = 1 .. 4: a cell missed in up to G
    # consecutive frames is linked to the cell that ended there, 2 .. G + 1 frames back, under the drift / flow summed over
    # the gap, and the table gains pred_gap (inference/cells.py)
    gap = None
    # [extension] cell_table: True = the table ends with the outline measures of every cell (perimeter, convex hull, Feret
    # length / width / angle; inference/cells.py)
    hull = False
    # [extension] cell_table: True = the table ends with the midline measures of every cell (the cell thinned to its
    # skeleton on the device; skeleton and midline length, end points; inference/cells.py)
    midline = False
    # [extension] cell_table: None = off; 1 .. 8 whole numbers in 0 .. 100, e.g. (5, 50, 95): the table ends with these
    # percentiles (50 = the median) of every cell's pixel values and of every frame's background per measured channel
    # (order statistics from the device; inference/cells.py)
    percentiles = None
    # [extension] cell_table: None = off; R, a whole number in 1 .. 32: the table ends with every cell's neighbourhood within
    # R pixels (contact edges, touching cells, nearest neighbour; contact_table gives the pairs; whole pixels, nothing beyond
    # R; inference/cells.py)
    neighbors = None
    # [extension] cell_table: None = off; THR, a whole number of grey levels in 1 .. 65535: the table ends with every cell's
    # fluorescent foci per measured channel (local maxima of an exact band-pass response of at least THR; spot_table gives the
    # spots; whole pixels, a fixed threshold; inference/cells.py); spot_scale: 1 .. 5, the size of the foci
    spots = None
    spot_scale = 2
    # [extension] cell_table: None = off; N, a whole number of bins in 2 .. 32: the table ends with where along the cell the
    # signal of every measured channel sits (pole-to-pole extent, pole / mid-cell ratio, pole asymmetry, brightest bin of the
    # intensity profile along the cell's orientation; profile_table gives the profiles; whole pixels, the straight axis;
    # inference/cells.py)
    profile = None
    # [extension] test-time augmentation (inference/tta.py): 1 = off (no existing route changes), 2 / 4 / 8 =
    # every frame is predicted under that many flips / rotations, the predictions are mapped back and averaged (fp32, in
    # member order) and the average is segmented: K network forwards per frame.  Whole-frame inference only
    tta = 1
    # [extension] inference at a chosen resolution (inference/resample.py): 1.0 = off (no existing route
    # changes), a real number in [0.25, 4] otherwise: every frame is resampled to out_size(H, scale) x out_size(W, scale) on
    # the device (anti-aliased linear), predicted there, the prediction is resampled back to H x W and segmented at the
    # frame's own resolution, so thresholds and seed sizes keep their meaning in original pixels.  Whole-frame inference
    # only, not together with tta
    scale = 1.0

    def __init__(self, img_id_list=None, inference_path=None, omero_username=None, omero_password=None, omero_host=None,
                 omero_port=None, group_id=None,
                 model=None, device='cuda:0', ths=(0.10, 0.45), channel=0, upload=True, overwrite=True,
                 sliding_window=False, print_output=False):
        super().__init__()
        self.img_id_list = img_id_list
        self.inference_path = inference_path
        self.omero_username, self.omero_password = omero_username, omero_password   # names: reference infer.py:30,66-69
        self.omero_host, self.omero_port, self.group_id = omero_host, omero_port, group_id
        self.model = model
        self.device = torch.device(device)
        self.ths = list(ths)           # [th_cell, th_seed] (infer.py:362-365)
        self.channel = channel
        self.upload = upload
        self.overwrite = overwrite
        # the reference stores this flag and never reads it (infer.py:60,76); here it switches on tiled inference, whose
        # prediction equals whole-frame inference (inference/tiling.py) and which lifts the 8192-px limit of the padding
        self.sliding_window = sliding_window
        self.print_output = print_output
        self.net, self.model_settings = (None, None)
        if model is not None:
            self.net, self.model_settings = load_model(model, self.device)

    def start_inference(self):
        """The reference pulls planes from an OMERO server here (infer.py:113-326): not part of this build."""
        raise RuntimeError("InferWorker.start_inference needs the OMERO stack (omero-py), which is outside the "
                           "MI355X hot path; use infer_stack()/inference() or infer_script_local.py")

    def pad_frame(self, img_frame, pad_val):
        """top / left padding of a frame up to the next tested shape, like the reference (utils.py:124-163).  Frames beyond
        8192 px raise 'Image too big to pad. Use sliding windows' there; with ``sliding_window`` they are padded to the
        16-px grid of the network instead (smaller frames keep the reference's padding, so that tiled and whole-frame
        inference see the same input)."""
        if self.sliding_window and max(img_frame.shape[:2]) > 8192:
            from .tiling import pad_to_grid
            return pad_to_grid(img_frame, pad_val)
        return zero_pad_model_input(img_frame, pad_val=pad_val)

    def inference(self, img, min_val, max_val, pads):
        """ Predict one (already padded) frame.

        :param img: padded frame (2-D numpy array, any integer/float dtype).
        :param min_val: minimum of the un-padded frame (numpy scalar of the image dtype).
        :param max_val: maximum of the un-padded frame.
        :param pads: [rows padded at the top, columns padded at the left] (removed after the forward pass).
        :return: instance mask, np.uint16, shape of the un-padded frame.
        """
        if self.scale != 1 or isinstance(self.scale, bool):     # the padding is the frame's own: the scaled frame gets its own
            return self._infer_stack_scaled(np.asarray(img)[None, pads[0]:, pads[1]:])[0]
        if self.tta != 1:               # the padding is the frame's own: every member is padded in its orientation
            return self._infer_stack_tta(np.asarray(img)[None, pads[0]:, pads[1]:])[0]
        self.net.eval()
        img_batch = normalize_host(img, min_val, max_val)
        img_batch = torch.from_numpy(np.ascontiguousarray(img_batch[None, None, :, :])).to(torch.float)
        with torch.no_grad():   # the reference disables autograd globally (infer.py:343); here only for the call
            pred = self._forward(img_batch)
            if pred is None:        # zero mask instead of a crash (infer.py:354-356) — out-of-memory only
                return np.zeros_like(img, dtype=np.uint16)[pads[0]:, pads[1]:]
            return self._postprocess(pred, pads).cpu().numpy().view(np.uint16)

    def _forward(self, img_batch):
        """network forward of one padded frame; None (after the reference's message) if it does not fit in memory"""
        try:
            with engine.precision_scope(self.precision):
                if isinstance(img_batch, engine.RawFrame):      # raw frame on the device: normalised by the first kernel
                    return self.net(img_batch)
                if self.sliding_window:
                    from .tiling import tiled_forward
                    return tiled_forward(self.net, img_batch.to(self.device), tile=self.tile_size)
                return self.net(img_batch.to(self.device))
        except (RuntimeError, MemoryError) as err:
            if not is_out_of_memory(err):
                raise
            self.text_output.emit('RuntimeError during inference (maybe not enough ram/vram?)')
            return None

    def _postprocess(self, pred, pads):
        """prediction (device) -> uint16 labels of the un-padded frame (device tensor, int16 storage)"""
        if self.model_settings['label_type'] == 'distance':
            border, cell = pred
            cell = cell[0, 0, pads[0]:, pads[1]:].contiguous()
            border = border[0, 0, pads[0]:, pads[1]:].contiguous()
            # every reference caller hands (H, W, 1) arrays to distance_postprocessing -> column-major instance ids
            labels, _, _ = pp.distance_postprocessing_device(border, cell, th_seed=self.ths[1], th_cell=self.ths[0],
                                                             col_major_ids=True)
        else:
            labels, _, _ = pp.boundary_postprocessing_device(self._softmax_hwc(pred, pads))
        return labels

    @staticmethod
    def _softmax_hwc(pred, pads):
        """(1, 3, Hp, Wp) logits -> (H, W, 3) softmax probabilities of the un-padded frame (device, current stream)"""
        lib = _lib.load()
        logits = pred.contiguous()
        _, _, hp, wp = logits.shape
        probs = torch.empty((hp - pads[0], wp - pads[1], 3), dtype=torch.float32, device=logits.device)
        _lib.check(lib.mseg_softmax3_hwc(logits.data_ptr(), hp, wp, int(pads[0]), int(pads[1]), probs.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "softmax3_hwc")
        return probs

    @staticmethod
    def _softmax_group(logits, pads):
        """contiguous (m, 3, Hp, Wp) logits -> (m, H, W, 3) softmax probabilities of the un-padded frames (current stream)"""
        lib = _lib.load()
        m, _, hp, wp = logits.shape
        probs = torch.empty((m, hp - pads[0], wp - pads[1], 3), dtype=torch.float32, device=logits.device)
        stream = torch.cuda.current_stream().cuda_stream
        for j in range(m):
            _lib.check(lib.mseg_softmax3_hwc(logits[j].data_ptr(), hp, wp, int(pads[0]), int(pads[1]), probs[j].data_ptr(),
                                             stream), "softmax3_hwc")
        return probs

    def _postprocess_group(self, pred, dst, pads):
        """Post-processing of a group's n frames, enqueued on the current stream; their masks go into the first n frames
        of ``dst`` ([>= n, H, W] int16 storage, pinned host memory or device).  ``pred``: distance models (border, cell),
        each [n, Hp, Wp] with the top / left ``pads`` still on; boundary models the frames' (H, W, 3) softmax
        probabilities one after the other (any iterable: a generator's softmax is enqueued right before the flood group
        that needs it), whose floods share a launch in groups of at most 8.  Returns the tensors that must stay alive
        until the current stream has passed this work."""
        if self.model_settings['label_type'] == 'distance':
            border, cell = pred
            # every reference caller hands (H, W, 1) arrays to distance_postprocessing -> column-major instance ids
            labels, _, _ = pp.distance_postprocessing_batch_device(border, cell, th_seed=self.ths[1], th_cell=self.ths[0],
                                                                   pads=pads, col_major_ids=True)
            dst[:labels.shape[0]].copy_(labels, non_blocking=True)
            return [border, cell, labels]
        keep, frames = [], iter(pred)
        for c0 in itertools.count(0, 8):
            probs = list(itertools.islice(frames, 8))
            if not probs:
                return keep
            outs = pp.boundary_postprocessing_batch_device(probs, first_slot=0)
            for i, (labels, _, _) in enumerate(outs):
                dst[c0 + i].copy_(labels, non_blocking=True)
            keep += [probs, outs]

    def _device_frames(self, frames, clahe):
        """[n, H, W] host frames -> (raw, minmax) on the device as ``tta.expand`` / ``resample.frames`` take them.  uint8 /
        uint16: uploaded raw (CLAHE first if asked for: uint16 from there on), minmax (n, 2) int32 reduced on the device;
        other dtypes: normalised per frame on the host as inference() does, float32, minmax None"""
        if frames.dtype in (np.uint8, np.uint16):
            n, H, W = frames.shape
            host = np.ascontiguousarray(frames)
            raw = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(self.device)
            if clahe:                                            # on the frames as recorded
                from ..utils.clahe import clahe_device
                raw = clahe_device(raw)
            minmax = torch.empty((n, 2), dtype=torch.int32, device=self.device)
            _lib.check(_lib.load().mseg_frames_minmax(raw.data_ptr(), engine.RawFrame.PIX[raw.dtype], n, H * W,
                                                      minmax.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "frames_minmax")
            return raw, minmax
        xs = [normalize_host(frame, np.min(frame), np.max(frame)).astype(np.float32) for frame in frames]
        return torch.from_numpy(np.ascontiguousarray(np.stack(xs))).to(self.device), None

    def _zero_failed(self, pred, failed):
        """zeros for the frames of a group's prediction (a tensor or a tuple of tensors, frames first) that did not fit"""
        if any(failed):
            bad = torch.tensor(failed, device=self.device)
            for t in (pred if isinstance(pred, tuple) else (pred,)):
                t[bad] = 0

    def _normalized_padded(self, frame):
        """one host frame -> (padded frame normalised with its own extrema, fp32, as inference() gets it; pads)"""
        frame_min, frame_max = np.min(frame), np.max(frame)
        padded, pads = self.pad_frame(np.copy(frame), frame_min)
        return normalize_host(padded, frame_min, frame_max), pads

    def _group_input(self, frames):
        """[n, H, W] host frames -> (network input (n, 1, Hp, Wp) fp32 on the device, pads).  uint8 / uint16: uploaded raw,
        extrema and normalisation / padding per frame on the device; other dtypes: per frame on the host as inference()"""
        if frames.dtype in (np.uint8, np.uint16) and max(frames.shape[1:]) <= 8192:
            from ..utils.utils import pad_amounts
            pads = pad_amounts(frames.shape[1:])
            host = np.ascontiguousarray(frames)
            raw = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(self.device)
            return engine.normalize_frames(raw, pads[0], pads[1]), pads
        xs, pads = [], [0, 0]
        for frame in frames:
            x, pads = self._normalized_padded(frame)
            xs.append(x)
        x = torch.from_numpy(np.ascontiguousarray(np.stack(xs)[:, None])).to(torch.float)
        return x.to(self.device), pads

    def forward_frames(self, frames):
        """[n, H, W] host array -> the network's prediction for the n frames from ONE forward at batch n, on the device
        (distance models: (border, cell), each (n, 1, Hp, Wp); boundary models: logits (n, 3, Hp, Wp); Hp x Wp = the padded
        frame).  Every frame is normalised with its own minimum / maximum."""
        frames = np.asarray(frames)
        if frames.ndim != 3:
            raise RuntimeError("forward_frames: a [n, H, W] array expected")
        self.net.eval()
        with torch.cuda.device(self.device), torch.no_grad():
            x, _ = self._group_input(frames)
            with engine.precision_scope(self.precision):
                return self.net(x)

    def _forward_group(self, x):
        """network forward of a group (n, 1, Hp, Wp) -> list of (first frame, frames, prediction or None): one entry unless
        the forward ran out of memory — then the group is halved and retried down to single frames, and a frame that does
        not fit alone gets None (zero mask, like inference())"""
        out, i, size = [], 0, x.shape[0]
        while i < x.shape[0]:
            m = min(size, x.shape[0] - i)
            try:
                with engine.precision_scope(self.precision):
                    pred = self.net(x[i:i + m])
            except (RuntimeError, MemoryError) as err:
                if not is_out_of_memory(err):
                    raise
                del err
                if self.device.type == 'cuda':
                    torch.cuda.empty_cache()          # cached blocks of the failed attempt must not starve the retry
                if m > 1:
                    size = max(1, m // 2)
                    continue
                self.text_output.emit('RuntimeError during inference (maybe not enough ram/vram?)')
                pred = None
            out.append((i, m, pred))
            i += m
        return out, size

    # -- [extension] test-time augmentation (inference/tta.py) ---------------------------------------------
    def _tta_member_codes(self):
        """member codes of ``self.tta``; raises before anything is launched if the route cannot take them"""
        from . import tta as T
        codes = T.member_codes(self.tta)
        if len(codes) > 1 and self.sliding_window:
            raise RuntimeError("test-time augmentation (tta > 1) needs whole-frame inference: tiled (sliding_window) "
                               "TTA is not implemented")
        if self.device.type != 'cuda':
            raise RuntimeError("test-time augmentation runs on the GPU: there is no CPU path")
        if self.model_settings is None or self.model_settings['label_type'] not in ('distance', 'boundary'):
            raise RuntimeError("test-time augmentation needs a distance or boundary model")
        return codes

    def predict_merged(self, frames):
        """[n, H, W] host array -> the merged prediction of the n frames on the device, without padding: distance models
        (border, cell), each (n, H, W); boundary models the softmax probabilities (n, H, W, 3).  The n frames are ONE
        group: per shape class their members go through the network member-major, in chunks of at most
        ``tta.chunk_members(...)[0]``; a frame with a member that did not fit in memory gets zeros."""
        return self._predict_merged(np.asarray(frames))[0]

    def _predict_merged(self, frames, clahe=False):
        """-> (merged prediction, [frame failed?])"""
        from ..utils.utils import pad_amounts
        from . import tta as T
        codes = self._tta_member_codes()
        if frames.ndim != 3 or frames.shape[0] == 0:
            raise RuntimeError("predict_merged: a [n, H, W] array expected")
        n, H, W = (int(v) for v in frames.shape)
        boundary = self.model_settings['label_type'] == 'boundary'
        self.net.eval()
        with torch.cuda.device(self.device), torch.no_grad():
            if frames.dtype in (np.uint8, np.uint16):
                pad_amounts((H, W))                              # frames beyond 8192 raise here, like every whole-frame route
            raw, minmax = self._device_frames(frames, clahe)     # (CLAHE on the un-transformed frames)
            failed = [False] * n
            members, keep = {}, []
            for cs, _, pads in T.shape_classes(codes, H, W):
                x = T.expand(raw, cs, pads, minmax)
                hp, wp = int(x.shape[2]), int(x.shape[3])
                x = x.view(len(cs) * n, 1, hp, wp)
                m, _ = T.chunk_members(hp, wp, self.frame_batch, len(codes))
                pieces = []
                for c0 in range(0, x.shape[0], m):
                    chunks, _ = self._forward_group(x[c0:c0 + m])
                    pieces += [(c0 + i, cnt, pred) for i, cnt, pred in chunks]
                pred = self._tta_join(pieces, n, failed, 3 if boundary else 1, hp, wp)
                if boundary:
                    logits = pred.contiguous()
                    probs = self._softmax_group(logits, pads)
                    keep += [logits, probs]
                    for ci, code in enumerate(cs):
                        members[code] = T.member(probs.permute(0, 3, 1, 2), code, first=ci * n)
                else:
                    keep += list(pred)
                    for ci, code in enumerate(cs):
                        members[code] = tuple(T.member(t, code, first=ci * n, pads=pads) for t in pred)
            order = sorted(members)
            if boundary:
                merged = T.merge([members[c] for c in order], n, 3, H, W, hwc=True)
            else:
                merged = tuple(T.merge([members[c][h] for c in order], n, 1, H, W)[:, 0] for h in (0, 1))
            del keep                                             # (alive until the merges were enqueued on this stream)
            self._zero_failed(merged, failed)
        return merged, failed

    def _tta_join(self, pieces, n, failed, ch, hp, wp):
        """the predictions of a class's members from the pieces its forwards came in; a piece that did not fit in memory
        becomes zeros and marks its frames (member j belongs to frame j % n)"""
        if len(pieces) == 1 and pieces[0][2] is not None:
            return pieces[0][2]
        heads = 1 if ch == 3 else 2
        parts = [[] for _ in range(heads)]
        for j0, cnt, pred in pieces:
            if pred is None:
                for j in range(j0, j0 + cnt):
                    failed[j % n] = True
                pred = tuple(torch.zeros((cnt, ch, hp, wp), dtype=torch.float32, device=self.device) for _ in range(heads))
            elif heads == 1:
                pred = (pred,)
            for h in range(heads):
                parts[h].append(pred[h])
        joined = tuple(torch.cat(p, dim=0) for p in parts)
        return joined[0] if heads == 1 else joined

    def _infer_stack_groups(self, img, group, predict):
        """infer_stack in groups of at most ``group`` frames, group after group on the main stream: ``predict(frames,
        clahe)`` -> (the group's prediction without padding, at the frames' resolution — distance models (border, cell),
        each (n, H, W); boundary models probabilities (n, H, W, 3) —, [frame failed?]), hook, the batched
        post-processing, masks back through one pinned buffer.  No side streams: nothing of a group overlaps the next.
        ``img`` holds at least one frame."""
        T_, H, W = (int(v) for v in img.shape)
        results = np.zeros(shape=(T_, H, W), dtype=np.uint16)
        boundary = self.model_settings['label_type'] == 'boundary'
        clahe = self._clahe_enabled(img)
        group = min(group, T_)
        with torch.cuda.device(self.device), torch.no_grad():
            host = torch.empty((group, H, W), dtype=torch.int16, pin_memory=True)
            for f0 in range(0, T_, group):
                if self.stop_inference:
                    break
                n = min(group, T_ - f0)
                pred, failed = predict(img[f0:f0 + n], clahe)
                if self.prediction_hook is not None:      # once per frame, in frame order, on the frame's own prediction
                    def hook(p, i):                       # (a frame that did not fit has no prediction: zero mask, no call)
                        return p if failed[i] else self.prediction_hook(p)
                    if boundary:
                        pred = torch.cat([hook(pred[i:i + 1].permute(0, 3, 1, 2), i).permute(0, 2, 3, 1)
                                          for i in range(n)], dim=0).contiguous()
                    else:
                        hooked = [hook((pred[0][i:i + 1, None], pred[1][i:i + 1, None]), i) for i in range(n)]
                        pred = (torch.cat([h[0] for h in hooked], dim=0)[:, 0], torch.cat([h[1] for h in hooked], dim=0)[:, 0])
                self._postprocess_group(pred, host, (0, 0))
                torch.cuda.current_stream().synchronize()
                results[f0:f0 + n] = host[:n].numpy().view(np.uint16)
                for i in range(n):
                    if failed[i]:
                        results[f0 + i] = 0
                    self.progress.emit(int(100 * (f0 + i + 1) / T_))
        return results

    def _infer_stack_tta(self, img):
        """infer_stack with ``tta > 1``: _infer_stack_groups over predict_merged (upload, expand, one forward per shape
        class and chunk, merge)"""
        from ..utils.utils import pad_amounts
        from . import tta as T
        codes = self._tta_member_codes()
        if len(img) == 0:
            return np.zeros(img.shape, dtype=np.uint16)
        pads = pad_amounts(img.shape[1:])
        _, group = T.chunk_members(img.shape[1] + pads[0], img.shape[2] + pads[1], self.frame_batch, len(codes))
        return self._infer_stack_groups(img, group, self._predict_merged)

    # -- [extension] inference at a chosen resolution (inference/resample.py) ------------------------------
    def _scale_checked(self):
        """``self.scale`` as a float; raises before anything is launched if the value or the route cannot be taken"""
        from . import resample as R
        s = R.check_scale(self.scale)
        if s != 1.0:
            if self.sliding_window:
                raise RuntimeError("inference at a chosen resolution (scale != 1) needs whole-frame inference: tiled "
                                   "(sliding_window) scaled inference is not implemented")
            if self.tta != 1:
                raise RuntimeError("inference at a chosen resolution (scale != 1) and test-time augmentation (tta > 1) "
                                   "are not implemented together")
        if self.device.type != 'cuda':
            raise RuntimeError("inference at a chosen resolution runs on the GPU: there is no CPU path")
        if self.model_settings is None or self.model_settings['label_type'] not in ('distance', 'boundary'):
            raise RuntimeError("inference at a chosen resolution needs a distance or boundary model")
        return s

    def _scaled_geometry(self, H, W, s):
        """-> ((Hs, Ws), pads of the scaled frame, y table, x table forwards, y table, x table back)"""
        from ..utils.utils import pad_amounts
        from . import resample as R
        hs, ws = R.out_size(H, s), R.out_size(W, s)
        pads = [int(p) for p in pad_amounts((hs, ws))]           # a scaled frame beyond 8192 raises here
        dev = self.device
        return (hs, ws), pads, R.axis(H, hs, dev), R.axis(W, ws, dev), R.axis(hs, H, dev), R.axis(ws, W, dev)

    def predict_scaled(self, frames):
        """[n, H, W] host array -> the prediction of the n frames on THEIR grid, without padding, on the device: distance
        models (border, cell), each (n, H, W); boundary models the softmax probabilities (n, H, W, 3).  The frames are
        resampled to ``scale`` on the device, go through the network as ONE group (halved if memory runs out) and the
        prediction is resampled back; a frame that did not fit in memory gets zeros."""
        return self._predict_scaled(np.asarray(frames))[0]

    def _predict_scaled(self, frames, clahe=False):
        """-> (prediction at the frames' resolution, [frame failed?])"""
        from . import resample as R
        s = self._scale_checked()
        if frames.ndim != 3 or frames.shape[0] == 0:
            raise RuntimeError("predict_scaled: a [n, H, W] array expected")
        n, H, W = (int(v) for v in frames.shape)
        boundary = self.model_settings['label_type'] == 'boundary'
        self.net.eval()
        with torch.cuda.device(self.device), torch.no_grad():
            _, pads, ydown, xdown, yup, xup = self._scaled_geometry(H, W, s)
            raw, minmax = self._device_frames(frames, clahe)
            x = R.frames(raw, ydown, xdown, pads, minmax)
            hp, wp = int(x.shape[1]), int(x.shape[2])
            chunks, _ = self._forward_group(x.view(n, 1, hp, wp))
            failed = [False] * n
            pred = self._tta_join(chunks, n, failed, 3 if boundary else 1, hp, wp)
            if boundary:
                out = R.planes(self._softmax_group(pred.contiguous(), pads).permute(0, 3, 1, 2), yup, xup, hwc=True)
            else:
                out = tuple(R.planes(t, yup, xup, pads=pads)[:, 0] for t in pred)
            self._zero_failed(out, failed)
        return out, failed

    def _infer_stack_scaled(self, img):
        """infer_stack with ``scale != 1``: _infer_stack_groups over predict_scaled (upload, resample, one forward,
        resample back), so the post-processing runs at the frame's resolution"""
        s = self._scale_checked()
        if len(img) == 0:
            return np.zeros(img.shape, dtype=np.uint16)
        (hs, ws), pads = self._scaled_geometry(int(img.shape[1]), int(img.shape[2]), s)[:2]
        group = frame_batch_for(hs + pads[0], ws + pads[1], self.frame_batch)
        return self._infer_stack_groups(img, group, self._predict_scaled)

    def _clahe_enabled(self, img):
        """apply_clahe for this stack?  Float stacks are segmented without it (no fixed grey-level range), with a message"""
        if not self.apply_clahe:
            return False
        if img.dtype not in (np.uint8, np.uint16):
            self.text_output.emit(f'Skip CLAHE (it needs uint8 / uint16 frames, got {img.dtype}): segmenting the frames as '
                                  'they are')
            return False
        if self.device.type != 'cuda':
            raise RuntimeError("apply_clahe runs on the GPU: there is no CPU path")
        return True

    def _clahe_host_frame(self, frame):
        """one host frame -> its CLAHE, uint16, back on the host (the routes that normalise on the host)"""
        from ..utils.clahe import equalize_adapthist_device
        with torch.cuda.device(self.device):
            return equalize_adapthist_device(np.ascontiguousarray(frame), device=self.device).cpu().numpy().view(np.uint16)

    def _infer_stack_batched(self, img, results, fb, boundary, clahe=False):
        """infer_stack with groups of ``fb`` frames: a group goes up through one of two pinned staging buffers on the copy
        stream, its forward (batch n) runs on the main stream, its post-processing — one batched call for distance models,
        the flood groups of at most 8 for boundary models — on the side stream, and its masks return through one pinned
        buffer per group in flight (reused once the group is done).  Tensors that another stream still reads are kept
        alive in ``pending`` until the group's event completed."""
        T = len(img)
        group_cap = fb
        device_norm = img.dtype in (np.uint8, np.uint16)
        from ..utils.utils import pad_amounts
        pads = pad_amounts(img.shape[1:])
        H, W = int(img.shape[1]), int(img.shape[2])
        side = torch.cuda.Stream(device=self.device, priority=-1) if boundary else torch.cuda.Stream(device=self.device)
        pending = []      # (first frame, frames, pinned host masks or None, event, tensors to keep alive)
        free_hosts = []   # pinned [fb, H, W] mask buffers, handed back by finish(): one per group in flight, reused

        def finish(entry):
            f0, n, host, ev, _keep = entry
            if ev is not None:
                ev.synchronize()
                results[f0:f0 + n] = host[:n].numpy().view(np.uint16)
                free_hosts.append(host)
            for f in range(f0, f0 + n):
                self.progress.emit(int(100 * (f + 1) / T))

        def launch_postproc(f0, n, pred):
            if self.prediction_hook is not None:
                pred = hook_per_frame(self.prediction_hook, pred)
            ready = torch.cuda.Event()
            ready.record()
            host = free_hosts.pop() if free_hosts else torch.empty((group_cap, H, W), dtype=torch.int16, pin_memory=True)
            with torch.cuda.stream(side):
                side.wait_event(ready)
                if boundary:
                    logits = pred.contiguous()
                    keep = [logits] + self._postprocess_group((self._softmax_hwc(logits[i:i + 1], pads) for i in range(n)),
                                                              host, pads)
                else:
                    keep = self._postprocess_group((pred[0][:, 0], pred[1][:, 0]), host, pads)
                done = torch.cuda.Event()
                done.record(side)
            pending.append((f0, n, host, done, keep))

        with torch.cuda.device(self.device), torch.no_grad():
            shape = (fb, H, W) if device_norm else (fb, 1, H + pads[0], W + pads[1])
            tdt = (torch.uint8 if img.dtype == np.uint8 else torch.int16) if device_norm else torch.float32
            stage = [torch.empty(shape, dtype=tdt, pin_memory=True) for _ in range(2)]
            dev_buf = [torch.empty(shape, dtype=tdt, device=self.device) for _ in range(2)]
            uploaded, consumed = [None, None], [None, None]
            copy_stream = torch.cuda.Stream(device=self.device)
            main = torch.cuda.current_stream()
            f0, g = 0, 0
            while f0 < T and not self.stop_inference:
                n = min(fb, T - f0)
                k = g & 1
                if uploaded[k] is not None:
                    uploaded[k].synchronize()                # the staging buffer is free again
                if device_norm:
                    np.copyto(stage[k][:n].numpy().view(img.dtype), img[f0:f0 + n])
                else:
                    dst = stage[k].numpy()
                    for i in range(n):
                        dst[i, 0] = self._normalized_padded(img[f0 + i])[0]
                with torch.cuda.stream(copy_stream):
                    if consumed[k] is not None:
                        copy_stream.wait_event(consumed[k])
                    dev_buf[k][:n].copy_(stage[k][:n], non_blocking=True)
                    uploaded[k] = torch.cuda.Event()
                    uploaded[k].record(copy_stream)
                main.wait_event(uploaded[k])
                if device_norm:
                    raw = dev_buf[k][:n]
                    if clahe:                                # one call for the group; uint16 frames from here on
                        from ..utils.clahe import clahe_device
                        raw = clahe_device(raw)
                    x = engine.normalize_frames(raw, pads[0], pads[1])
                else:
                    x = dev_buf[k][:n]
                chunks, size = self._forward_group(x)
                consumed[k] = torch.cuda.Event()
                consumed[k].record(main)
                fb = min(fb, size)                           # after an out-of-memory: smaller groups from here on
                for c0, m, pred in chunks:
                    if pred is None:
                        pending.append((f0 + c0, m, None, None, None))
                    else:
                        launch_postproc(f0 + c0, m, pred)
                while len(pending) > 2:                      # two groups in flight
                    finish(pending.pop(0))
                f0 += n
                g += 1
            while pending:
                finish(pending.pop(0))
        return results

    def infer_stack(self, img):
        """[T, H, W] stack -> [T, H, W] uint16 masks; per frame min/max + top/left padding exactly like
        infer_script_local.py:118-161 / infer.py:250-259.

        MI355X path for distance models: the frames are pipelined over two HIP streams — while the watershed of frame i
        (a few long-running, latency-bound lanes) runs on the side stream, the matrix kernels of frame i+1 run on the
        main stream, and the uint16 mask travels back through a pinned buffer.  Results are identical to calling
        ``inference`` frame by frame."""
        if self.scale != 1 or isinstance(self.scale, bool):
            return self._infer_stack_scaled(img)
        if self.tta != 1:
            return self._infer_stack_tta(img)
        results = np.zeros(shape=(img.shape[0], img.shape[1], img.shape[2]), dtype=np.uint16)
        pipelined = (self.model_settings is not None and self.model_settings['label_type'] in ('distance', 'boundary')
                     and self.device.type == 'cuda')
        boundary = pipelined and self.model_settings['label_type'] == 'boundary'
        clahe = self._clahe_enabled(img)
        if pipelined and int(self.frame_batch) != 1 and len(img) > 0:
            if self.sliding_window:
                self.text_output.emit('frame_batch is ignored with sliding-window inference')
            elif max(img.shape[1:]) <= 8192:
                from ..utils.utils import pad_amounts
                pads = pad_amounts(img.shape[1:])
                fb = frame_batch_for(img.shape[1] + pads[0], img.shape[2] + pads[1], self.frame_batch)
                if fb > 1:
                    self.net.eval()
                    return self._infer_stack_batched(img, results, fb, boundary, clahe)
        if not pipelined:
            for frame in range(len(img)):
                if self.stop_inference:
                    break
                img_frame = self._clahe_host_frame(img[frame]) if clahe else np.copy(img[frame])
                frame_min, frame_max = np.min(img_frame), np.max(img_frame)
                img_frame, pads = self.pad_frame(img_frame, frame_min)
                results[frame] = self.inference(img_frame, frame_min, frame_max, pads)
                self.progress.emit(int(100 * (frame + 1) / len(img)))
            return results

        self.net.eval()
        # Side streams for the post-processing.  Distance method: one (the watershed of frame i under the network of frame
        # i + 1).  Boundary method: its flood is ONE wavefront busy for ~45 ms per 2048^2 frame (the heap's
        # marker phase is sequential by definition) — a latency, not a load.  The frames of a stack are collected in groups of
        # BOUNDARY_BATCH and a group's floods go into ONE launch, one workgroup per frame (mseg_boundary_flood_batch: eight
        # floods take the time of one); two side streams alternate between groups, each group on its own workspace slots,
        # while the network goes on with the next frames.  HIGH-priority streams: HIP multiplexes streams onto a few hardware
        # queues per priority level and kernels of streams that share a queue run one after the other — at the default
        # priority a 45-ms flood sat in front of the network's kernels whenever its stream shared the main stream's queue.
        batch = max(1, min(int(self.BOUNDARY_BATCH), 8)) if boundary else 1
        if boundary:      # two groups' workspaces (0.32 GiB per 2048^2 frame, 5.2 GiB per 8192^2 frame) stay below ~16 GiB
            per_frame = max(1, _lib.load().mseg_postproc_workspace_bytes(int(img.shape[1]), int(img.shape[2])))
            batch = max(1, min(batch, (8 << 30) // per_frame))
        nside = 2 if boundary else 1
        sides = [torch.cuda.Stream(device=self.device, priority=-1) if boundary else torch.cuda.Stream(device=self.device)
                 for _ in range(nside)]
        in_flight = 2 * batch if boundary else 2
        pending = []      # (frame index, pinned host mask, event on the side stream)
        group, groups_done = [], [0]

        def finish(entry):
            f, host, ev = entry
            if ev is not None:
                ev.synchronize()
                results[f] = host.numpy().view(np.uint16)
            self.progress.emit(int(100 * (f + 1) / len(img)))

        def flush_group():
            """boundary method: softmax + post-processing of the collected frames on one side stream, their floods in one launch"""
            if not group:
                return
            side = sides[groups_done[0] % nside]
            slot0 = (groups_done[0] % nside) * 8
            groups_done[0] += 1
            ready = torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(side):
                side.wait_event(ready)
                outs = pp.boundary_postprocessing_batch_device([self._softmax_hwc(lg, pads) for _, lg, pads in group],
                                                               first_slot=slot0)
                for (frame, lg, _), (labels, _, _) in zip(group, outs):
                    lg.record_stream(side)
                    host = torch.empty(labels.shape, dtype=torch.int16, pin_memory=True)
                    host.copy_(labels, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(side)
                    pending.append((frame, host, done))
            group.clear()

        def launch_postproc(frame, pred, pads):
            if self.prediction_hook is not None:
                pred = self.prediction_hook(pred)
            if boundary:
                group.append((frame, pred.contiguous(), pads))
                if len(group) >= batch:
                    flush_group()
                return
            side = sides[0]
            border, cell = pred
            cell = cell[0, 0, pads[0]:, pads[1]:].contiguous()
            border = border[0, 0, pads[0]:, pads[1]:].contiguous()
            ready = torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(side):
                side.wait_event(ready)
                labels, _, _ = pp.distance_postprocessing_device(border, cell, th_seed=self.ths[1],
                                                                 th_cell=self.ths[0], col_major_ids=True)
                border.record_stream(side)
                cell.record_stream(side)
                host = torch.empty(labels.shape, dtype=torch.int16, pin_memory=True)
                host.copy_(labels, non_blocking=True)
                done = torch.cuda.Event()
                done.record(side)
            pending.append((frame, host, done))

        # K14 on the device (uint8 / uint16 stacks, whole-frame inference): the raw frame goes up from a pinned staging
        # buffer on a copy stream, its extrema are reduced on the device and the first convolution normalises / pads while it
        # loads (engine.RawFrame) — the host loop only copies into pinned memory and enqueues.  Same input values bit for
        # bit as the host formula of inference() (tests/test_gpu_fullsize.py), so the masks are identical.
        device_norm = (img.dtype in (np.uint8, np.uint16) and not self.sliding_window and img.shape[1] <= 8192
                       and img.shape[2] <= 8192)
        with torch.cuda.device(self.device), torch.no_grad():
            if device_norm:
                from ..utils.utils import pad_amounts
                pads = pad_amounts(img.shape[1:])
                tdt = torch.uint8 if img.dtype == np.uint8 else torch.int16      # (uint16 bits in int16 storage)
                stage = [torch.empty(img.shape[1:], dtype=tdt, pin_memory=True) for _ in range(2)]
                raw_dev = [torch.empty(img.shape[1:], dtype=tdt, device=self.device) for _ in range(2)]
                uploaded = [None, None]          # copy-stream events: staging buffer k has left the host
                consumed = [None, None]          # main-stream events: the network has read device buffer k
                copy_stream = torch.cuda.Stream(device=self.device)
                main = torch.cuda.current_stream()
            for frame in range(len(img)):
                if self.stop_inference:
                    break
                if device_norm:
                    k = frame & 1
                    if uploaded[k] is not None:
                        uploaded[k].synchronize()            # the staging buffer is free again
                    np.copyto(stage[k].numpy().view(img.dtype), img[frame])
                    with torch.cuda.stream(copy_stream):
                        if consumed[k] is not None:
                            copy_stream.wait_event(consumed[k])
                        raw_dev[k].copy_(stage[k], non_blocking=True)
                        uploaded[k] = torch.cuda.Event()
                        uploaded[k].record(copy_stream)
                    main.wait_event(uploaded[k])
                    raw = raw_dev[k]
                    if clahe:                            # enhanced on the main stream; a uint16 frame from here on
                        from ..utils.clahe import clahe_device
                        raw = clahe_device(raw[None])[0]
                    pred = self._forward(engine.RawFrame(raw, pads[0], pads[1]))
                    consumed[k] = torch.cuda.Event()
                    consumed[k].record(main)
                else:
                    # (sliding-window inference comes here: the whole frame is enhanced before it is tiled)
                    img_frame = self._clahe_host_frame(img[frame]) if clahe else np.copy(img[frame])
                    frame_min, frame_max = np.min(img_frame), np.max(img_frame)
                    img_frame, pads = self.pad_frame(img_frame, frame_min)
                    img_batch = normalize_host(img_frame, frame_min, frame_max)
                    img_batch = torch.from_numpy(np.ascontiguousarray(img_batch[None, None, :, :])).to(torch.float)
                    pred = self._forward(img_batch)
                if pred is None:                 # out of memory: zero mask, like inference() (infer.py:354-356)
                    pending.append((frame, None, None))
                else:
                    launch_postproc(frame, pred, pads)
                while len(pending) > in_flight:  # distance: two frames in flight; boundary: two groups
                    finish(pending.pop(0))
            flush_group()
            while pending:
                finish(pending.pop(0))
        return results

    # -- what follows the prediction on the reference's routes (infer.py:265-291 upload, :320-322 local save) -------------
    STROKE_COLOR = int.from_bytes([255, 255, 0, 255], byteorder='big', signed=True)     # yellow, opaque (infer.py:271-272)

    def polygon_rois(self, prediction, frame=0):
        """ One polygon ROI per cell of a predicted frame, as plain records with the fields the reference sets on its
        ``omero.model.PolygonI`` objects (theZ, theT, theC, fillColor, strokeColor, points = "x,y x,y ... ").  The
        contours of ALL instances are traced on the device in two launches (utils/hull_polygon.py) instead of one
        ``cv2.findContours`` call per instance. """
        from ..utils.hull_polygon import label_polygons, points_string
        rois = []
        if np.max(prediction) > 0:
            for polygons in label_polygons(prediction).values():
                for polygon in polygons:
                    rois.append({'theZ': 0, 'theT': int(frame), 'theC': int(self.channel), 'fillColor': 0,
                                 'strokeColor': self.STROKE_COLOR, 'points': points_string(polygon)})
        return rois

    def cell_table(self, results, img=None, channels=None):
        """ [extension] The per-cell table of a segmented stack (inference/cells.py ``measure_cells``): ``results`` are the
        masks of ``infer_stack``, ``img`` the [T, C, H, W] image (a strided view is read in place) whose ``channels``
        (numbers of the source image, they name the columns) are measured.  Overlap linking: no motion model, no gap
        closing unless ``self.gap`` is set (then across up to that many missed frames); with ``self.drift`` set, under the
        estimated stage drift of every frame pair; with ``self.flow`` set as well, under a
        tile-wise displacement field around it (tiles of ``self.flow_tile`` pixels); with ``self.hull`` set, with
        the outline columns; with ``self.midline`` set, with the midline columns; with ``self.percentiles`` set, with the
        percentile columns; with ``self.neighbors`` set, with the neighbourhood columns; with ``self.spots`` set, with the
        spot columns at ``self.spot_scale``; with ``self.profile`` set, with the profile columns of that many bins. """
        from .cells import channel_stems, measure_cells
        df = measure_cells(results, img, link=True, min_overlap=self.min_overlap, device=self.device, drift=self.drift,
                           hull=self.hull, midline=self.midline, percentiles=self.percentiles, neighbors=self.neighbors,
                           spots=self.spots, spot_scale=self.spot_scale, flow=self.flow, flow_tile=self.flow_tile,
                           gap=self.gap, profile=self.profile)
        if img is not None and channels is not None:      # the view holds the chosen channels only: name them by source
            names = {f'{k}_ch{i}': f'{k}_ch{int(c)}' for i, c in reversed(list(enumerate(channels)))
                     for k in channel_stems(self.percentiles or (), self.spots is not None, self.profile is not None)}
            df = df.rename(columns=names)
        return df

    def spot_table(self, results, img, channels=None):
        """ [extension] The fluorescent foci of a segmented stack (inference/cells.py ``cell_spots``): one row per spot of at
        least ``self.spots`` grey levels at ``self.spot_scale``, with the cell it lies on and its position along the cell's
        axes.  ``img`` as for ``cell_table``; ``channels``: the numbers of the source image the view's channels have (they
        go into the ``channel`` column).  Whole pixels, a fixed threshold; spots on the background are left out. """
        from .cells import cell_spots
        df = cell_spots(results, img, spots=self.spots, spot_scale=self.spot_scale, device=self.device)
        if channels is not None:
            df['channel'] = df['channel'].map(lambda i: int(channels[i]))
        return df

    def profile_table(self, results, img, channels=None):
        """ [extension] The intensity profiles of a segmented stack along every cell's axis (inference/cells.py
        ``cell_profiles``): one row per cell, channel and bin of ``self.profile`` bins.  ``img`` as for ``cell_table``;
        ``channels``: the numbers of the source image the view's channels have (they go into the ``channel`` column).  Whole
        pixels, along the straight orientation axis; no background subtraction. """
        from .cells import cell_profiles
        df = cell_profiles(results, img, bins=self.profile, device=self.device)
        if channels is not None:
            df['channel'] = df['channel'].map(lambda i: int(channels[i]))
        return df

    def contact_table(self, results):
        """ [extension] The contact graph of a segmented stack (inference/cells.py ``cell_contacts``): one row per pair of
        cells of one frame within ``self.neighbors`` pixels of each other, with the pixel edges they share and their
        distance.  Whole pixels, centre-to-centre; nothing beyond that radius. """
        from .cells import cell_contacts
        return cell_contacts(results, self.neighbors, self.device)

    def save_results(self, results_array, image_name, result_path=None, with_rois=False):
        """ ``<result_path>/<image stem>_channel<c>.tif`` (uint16 [T, H, W], the reference's local-save route) and, with
        ``with_rois``, ``<...>_rois.json``: the polygon ROIs per frame that the upload route would send to OMERO. """
        from ..utils import tiffio as tiff
        result_path = Path(self.inference_path if result_path is None else result_path)
        result_path.mkdir(parents=True, exist_ok=True)
        stem = Path(image_name).stem
        target = result_path / f"{stem}_channel{self.channel}.tif"
        tiff.imwrite(str(target), results_array)
        if with_rois:
            frames = results_array if results_array.ndim == 3 else results_array[None]
            rois = [roi for t, frame in enumerate(frames) for roi in self.polygon_rois(frame, t)]
            with open(result_path / f"{stem}_channel{self.channel}_rois.json", 'w', encoding='utf-8') as f:
                json.dump({'image': str(image_name), 'channel': int(self.channel), 'rois': rois}, f)
        return target

    @pyqtSlot()
    def inference_finished(self):
        self.finished.emit()

    @pyqtSlot()
    def stop_inference_process(self):
        """ Set internal stop state to True """
        self.stop_inference = True
