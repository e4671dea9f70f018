"""numpy restatement of the reference's training-set preparation (src/utils/data_cropping.py:157-264,286,
src/utils/data_import.py:125-194, src/utils/data_export.py:100-101), written on arrays the way the reference works on them
(it pads the image, then reads the padded array's shape), independently of microbeseg_amd/utils/data_cropping.py and
data_import.py.  The tests call it for random inputs; tools/gen_golden_prepare.py stores its results, together with what
only scikit-image can provide (polygon / polygon_perimeter), in tests/golden/prepare_*.npz."""
import numpy as np

SHAPES = [(60, 75), (64, 64), (60, 60), (75, 225), (225, 75), (140, 100), (60, 200), (193, 64), (64, 193), (58, 300),
          (50, 50)]


def frame_for(shape, dtype, seed):
    """a test frame: smooth blobs plus noise over most of the dtype's range, never constant"""
    rng = np.random.Generator(np.random.PCG64(seed))
    top = np.iinfo(dtype).max
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    base = 0.5 + 0.4 * np.sin(yy / 9.0 + seed) * np.cos(xx / 7.0)
    img = np.clip(base * 0.8 * top + rng.normal(0, 0.02 * top, shape) + 0.05 * top, 0, top)
    return img.astype(dtype)


def origins_ref(img, crop_size, rng):
    """data_cropping.py:157-199 -> None (frame skipped) or (padded image, [(a, b), ...]); rng: random.Random"""
    crop_dim = 0 if img.shape[0] > img.shape[1] else 1
    n_crops = 3 if img.shape[crop_dim] > 3 * crop_size else (2 if img.shape[crop_dim] > 2 * crop_size else 1)
    img_min = np.min(img)
    if 0.9 * crop_size > img.shape[0] or 0.9 * crop_size > img.shape[1]:
        return None
    x_pads = np.maximum(0, crop_size - img.shape[1])
    y_pads = np.maximum(0, crop_size - img.shape[0])
    img = np.pad(img, ((0, y_pads), (0, x_pads)), mode='constant', constant_values=img_min)
    out = []
    for i in range(n_crops):
        c = img.shape[crop_dim] // n_crops
        a, b = 0, 0
        if x_pads > 0:
            pass
        elif crop_dim == 0 and y_pads == 0 and img.shape[0] > crop_size:
            a = rng.randint(i * c, int(np.minimum(img.shape[0] - crop_size, (i + 1) * c - crop_size)))
            b = rng.randint(0, img.shape[1] - crop_size)
        elif crop_dim == 1 and img.shape[1] > crop_size:
            a = rng.randint(0, img.shape[0] - crop_size)
            b = rng.randint(i * c, int(np.minimum(img.shape[1] - crop_size, (i + 1) * c - crop_size)))
        out.append((a, b))
    return img, out


def crop_views(padded, origins, crop_size, lo, hi):
    """-> (img, img_show, x, u16) per data_cropping.py:202-206,261,286 and data_export.py:100-101; lo / hi are scalars of
    the image dtype (cropping) or Python ints (export)"""
    imgs, shows, xs, u16s = [], [], [], []
    for a, b in origins:
        crop = padded[a:a + crop_size, b:b + crop_size]
        imgs.append(crop)
        with np.errstate(all='ignore'):
            shows.append((255 * (crop.astype(np.float32) - lo) / (hi - lo)).astype(np.uint8))
        xs.append(2 * (crop.astype(np.float32) - lo) / (hi - lo) - 1)
        u = 65535 * (crop.astype(np.float32) - int(lo)) / (int(hi) - int(lo))
        u16s.append(np.clip(u, 0, 65535).astype(np.uint16))
    return np.stack(imgs), np.stack(shows), np.stack(xs).astype(np.float32), np.stack(u16s)


def pad_to_crop(img, crop_size, value):
    """bottom / right padding of data_cropping.py:178-180"""
    return np.pad(img, ((0, max(0, crop_size - img.shape[0])), (0, max(0, crop_size - img.shape[1]))), mode='constant',
                  constant_values=value)


def census_ref(mask, y0, x0, ny, nx, crop_size):
    """per crop of the grid and, last, for the region: (distinct non-zero ids, non-zero pixels)"""
    cells, area = [], []
    region = mask[y0:y0 + ny * crop_size, x0:x0 + nx * crop_size]
    for h in range(ny):
        for w in range(nx):
            crop = region[h * crop_size:(h + 1) * crop_size, w * crop_size:(w + 1) * crop_size]
            ids = np.unique(crop)
            cells.append(int((ids > 0).sum()))
            area.append(int(np.sum(crop > 0)))
    ids = np.unique(region)
    return np.asarray(cells + [int((ids > 0).sum())], np.int64), np.asarray(area + [int(np.sum(region > 0))], np.int64)


def import_ref(img, mask, crop_size, keep_normalization):
    """data_import.py:125-185 for one image / mask pair that passed the file checks -> None ("too much pads") or a dict:
    min_frame, max_frame, mean_frame, std_frame, crops = [(img_crop, mask_crop, x_start, y_start), ...] (accepted, in
    order), rejected_empty / rejected_small = numbers of crops each rule threw out"""
    if keep_normalization and np.issubdtype(img.dtype, np.unsignedinteger):
        min_frame, max_frame = np.iinfo(img.dtype).min, np.iinfo(img.dtype).max
    else:
        min_frame, max_frame = np.min(img), np.max(img)
    mean_frame, std_frame = np.mean(img), np.std(img)
    pads = [max(0, crop_size - img.shape[0]), max(0, crop_size - img.shape[1])]
    if pads[0] > img.shape[0] or pads[1] > img.shape[1]:
        return None
    widths = ((int(np.ceil(pads[0] / 2)), int(np.floor(pads[0] / 2))), (int(np.ceil(pads[1] / 2)), int(np.floor(pads[1] / 2))))
    img, mask = np.pad(img, widths, mode='constant'), np.pad(mask, widths, mode='constant')
    out = dict(min_frame=min_frame, max_frame=max_frame, mean_frame=mean_frame, std_frame=std_frame, crops=[],
               rejected_empty=0, rejected_small=0)
    if img.shape[0] > crop_size or img.shape[1] > crop_size:
        ny, nx = img.shape[0] // crop_size, img.shape[1] // crop_size
        border_y = np.maximum(0, (img.shape[0] - ny * crop_size) / 2)
        border_x = np.maximum(0, (img.shape[1] - nx * crop_size) / 2)
        if border_y > 0:
            img = img[int(np.floor(border_y)):int(np.floor(-border_y)), ...]
            mask = mask[int(np.floor(border_y)):int(np.floor(-border_y)), ...]
        if border_x > 0:
            img = img[:, int(np.floor(border_x)):int(np.floor(-border_x))]
            mask = mask[:, int(np.floor(border_x)):int(np.floor(-border_x))]
        ids = np.unique(mask)
        num_cells, area_cells = int((ids > 0).sum()), np.sum(mask > 0)
        for h in range(ny):
            for w in range(nx):
                ys, xs = h * crop_size, w * crop_size
                mc = mask[ys:ys + crop_size, xs:xs + crop_size]
                n_crop = int((np.unique(mc) > 0).sum())
                if n_crop == 0:
                    out['rejected_empty'] += 1
                    continue
                if np.sum(mc > 0) < area_cells / num_cells:
                    out['rejected_small'] += 1
                    continue
                out['crops'].append((np.copy(img[ys:ys + crop_size, xs:xs + crop_size]), np.copy(mc),
                                     xs + int(np.floor(border_x)), ys + int(np.floor(border_y))))
    else:
        out['crops'].append((np.copy(img), np.copy(mask), 0, 0))
    return out


def export_image_ref(img_crop, min_frame, max_frame):
    """data_export.py:84-86,100-101: the stored strings parsed as ints, multiply before divide in float32"""
    frame_min, frame_max = int(str(min_frame)), int(str(max_frame))
    img = 65535 * (img_crop.astype(np.float32) - frame_min) / (frame_max - frame_min)
    return np.clip(img, 0, 65535).astype(np.uint16)


def overlay_ref(show, outlines):
    """data_cropping.py:214-215,238-240"""
    rgb = np.concatenate((show[..., None], show[..., None], show[..., None]), axis=-1)
    rgb[outlines, 0] = 255
    rgb[outlines, 1] = 255
    rgb[outlines, 2] = 0
    return rgb


def cell_mask(shape, cells, seed):
    """label image with the given (id, cy, cx, ry, rx) ellipses, later ids on top"""
    m = np.zeros(shape, np.uint16)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    for i, cy, cx, ry, rx in cells:
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = i
    return m
