#!/opt/conda/bin/python3.9
"""Generate tests/golden/analysis_*.npz with the REAL reference Analysis / Export loops (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 -W ignore tools/gen_golden_analysis.py
Imports AnalysisWorker (/root/reference/src/inference/analysis.py) and ResultExportWorker
(/root/reference/src/inference/result_export.py) unchanged and runs analyze_data() / export_data() against an in-memory
stand-in of the OMERO server: placeholder modules for omero, omero.model (PolygonI is a class: the loops test
``type(s) == omero.model.PolygonI``), omero.gateway, omero.rtypes and PyQt5.QtCore, and a fake connection that serves the
image planes and the polygon shapes and captures the CSV handed to createFileAnnfromLocalFile.  The conda env has
scikit-image 0.18.3, whose RegionProperties names the axes major_axis_length / minor_axis_length; the reference reads
axis_major_length / axis_minor_length (the 0.19 names of the same properties), so those two aliases are added.
tifffile 2021.7.2 writes the export files, which are read back.  Only inputs (image stack, ROI strings in iteration order,
their frames) and the reference's outputs (CSV text, mask, outlines, overlay, messages) are stored.
"""
import pathlib
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = pathlib.Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "golden"
CURRENT = {}


def _install_placeholders():
    sys.path.insert(0, str(ROOT))
    from microbeseg_amd.utils import qt_shim
    omero = types.ModuleType("omero")
    model = types.ModuleType("omero.model")
    gateway = types.ModuleType("omero.gateway")
    rtypes = types.ModuleType("omero.rtypes")

    class PolygonI:
        def __init__(self, t, points):
            self._t, self._p = t, points

        def getTheT(self):
            return types.SimpleNamespace(getValue=lambda: self._t)

        def getPoints(self):
            return types.SimpleNamespace(getValue=lambda: self._p)

    class ProjectWrapper:
        pass

    model.PolygonI = PolygonI
    gateway.ProjectWrapper = ProjectWrapper
    gateway.BlitzGateway = lambda *a, **k: FakeConn(CURRENT["image"])   # the image of the case being run
    omero.model, omero.gateway, omero.rtypes = model, gateway, rtypes
    qtcore = types.ModuleType("PyQt5.QtCore")
    for n in ("QObject", "pyqtSignal", "pyqtSlot", "QCoreApplication"):
        setattr(qtcore, n, getattr(qt_shim, n))
    pyqt = types.ModuleType("PyQt5")
    pyqt.QtCore = qtcore
    sys.modules.update({"omero": omero, "omero.model": model, "omero.gateway": gateway, "omero.rtypes": rtypes,
                        "PyQt5": pyqt, "PyQt5.QtCore": qtcore})
    from skimage.measure._regionprops import RegionProperties
    if not hasattr(RegionProperties, "axis_major_length"):
        RegionProperties.axis_major_length = property(lambda s: s.major_axis_length)
        RegionProperties.axis_minor_length = property(lambda s: s.minor_axis_length)
    return PolygonI


class FakeImage:
    def __init__(self, img, C, shapes, name, csv_store):
        self.img, self.C, self.shapes, self.name, self.csv = img, C, shapes, name, csv_store
        self.T, self.H, self.W = img.shape[:3]

    def getId(self): return 1
    def getName(self): return self.name
    def listParents(self): return [None]
    def getProject(self): return types.SimpleNamespace(getName=lambda: "proj")
    def getSizeT(self): return self.T
    def getSizeY(self): return self.H
    def getSizeX(self): return self.W
    def getSizeC(self): return self.C
    def getSizeZ(self): return 1
    def getPixelsType(self): return str(self.img.dtype)
    def linkAnnotation(self, ann): pass

    def getPrimaryPixels(self):
        def planes(zct):
            for z, c, t in zct:
                yield self.img[t] if self.C == 1 else self.img[t, :, :, c]
        return types.SimpleNamespace(getPlanes=planes)

    def listAnnotations(self, ns=None):
        if "text" not in self.csv:
            return []
        data = self.csv["text"]
        return [types.SimpleNamespace(getId=lambda: 1, getFileInChunks=lambda: iter([data]))]


class FakeConn:
    def __init__(self, image):
        self.image = image

    def connect(self): return True
    def setGroupForSession(self, g): pass
    def close(self): pass
    def getObject(self, kind, i): return self.image
    def canWrite(self, img): return True
    def deleteObjects(self, *a, **k): pass

    def getRoiService(self):
        rois = [types.SimpleNamespace(copyShapes=lambda s=s: list(s)) for s in self.image.shapes]
        return types.SimpleNamespace(findByImage=lambda i, o: types.SimpleNamespace(rois=rois))

    def createFileAnnfromLocalFile(self, path, mimetype=None, ns=None, desc=None):
        self.image.csv["text"] = pathlib.Path(path).read_bytes()
        return object()


def pts(r, c, jitter=None):
    """ROI string "x,y x,y " (the format InferWorker.polygon_rois writes), optionally with non-integer coordinates"""
    s = ""
    for i, (y, x) in enumerate(zip(r, c)):
        if jitter is not None:
            y, x = y + jitter[i, 0], x + jitter[i, 1]
            s += f"{x:.2f},{y:.2f} "
        else:
            s += f"{int(x)},{int(y)} "
    return s


def case_mixed(rng):
    T, H, W = 3, 48, 64
    rois = []   # (t, points)
    rois.append((0, pts([-3, 10, 20, 5], [-2, -5, 12, 30])))                 # touches the top / left border (clamped)
    rois.append((0, pts([30, 52, 52], [50, 70, 40])))                        # bottom / right border
    rois.append((0, pts([10, 10, 25, 25], [20, 35, 35, 20])))                # square ...
    rois.append((0, pts([15, 15, 30, 30], [28, 45, 45, 28])))                # ... overlapped by a later one
    rois.append((0, pts([30, 30, 40, 40], [5, 15, 15, 5])))                  # touching, different ids
    rois.append((0, pts([30, 30, 40, 40], [16, 25, 25, 16])))
    rois.append((2, pts([5, 20, 5, 20], [5, 20, 20, 5])))                    # self-intersecting bow tie
    rois.append((2, pts([25, 25, 25, 30, 35, 35, 35, 30], [5, 10, 15, 15, 15, 10, 5, 5])))   # collinear vertices
    rois.append((2, pts([8, 8, 8, 14, 20, 20, 14], [30, 30, 40, 44, 40, 30, 30])))           # duplicate vertices
    rois.append((2, pts([1, 9, 5, 2], [40, 43, 58, 41])))
    rois.append((2, pts([26, 44, 40, 30, 44], [30, 33, 55, 62, 40])))        # star-ish, self-intersecting
    for _ in range(6):                                                       # random non-integer polygons
        n = int(rng.integers(3, 9))
        cy, cx = rng.uniform(5, H - 5), rng.uniform(5, W - 5)
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        rad = rng.uniform(2, 9, n)
        r, c = cy + rad * np.sin(a), cx + rad * np.cos(a)
        rois.append((int(rng.choice([0, 2])), pts(np.floor(r), np.floor(c), jitter=np.c_[r % 1, c % 1])))
    img = (rng.integers(0, 4000, (T, H, W))).astype(np.uint16)
    return img, 1, rois


def case_rgb(rng):
    T, H, W = 2, 40, 40
    rois = []
    for t in range(T):
        for _ in range(8):
            n = int(rng.integers(3, 12))
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            a = np.sort(rng.uniform(0, 2 * np.pi, n))
            rad = rng.uniform(2, 10, n)
            rois.append((t, pts(np.round(cy + rad * np.sin(a)), np.round(cx + rad * np.cos(a)))))
    img = rng.integers(0, 200, (T, H, W, 3)).astype(np.uint8)
    return img, 3, rois


def case_wrap(rng):
    """66 600 polygons: cell ids 65536..66534 wrap to 0..998 in the uint16 stack (0 erases part of cell 400, the others
    merge with the equal-valued early cell they touch), from 66535 on the stack is int32"""
    T, H, W = 2, 64, 64
    n_total = 66600
    slot = lambda k: ((k % 400) // 20 * 3 + 1, (k % 400) % 20 * 3 + 1)   # noqa: E731  3x3 slots, 400 per frame
    rois = []
    for k in range(1, n_total + 1):
        if k <= 1200:
            t = 0 if k <= 400 else 1
            y, x = slot(k)
            rois.append((t, pts([y, y, y + 1], [x, x + 1, x])))
        elif k < 65536:
            rois.append((1, pts([61, 61, 62], [61, 62, 61])))               # repeatedly overwritten
        elif k == 65536:                                                    # wraps to 0: erases pixel (1, 1) of cell 400
            rois.append((0, pts([1, 1, 2], [0, 1, 0])))
        else:
            v = k - 65536                                                   # wrapped value
            y, x = slot(v)
            t = 0 if v <= 400 else 1
            rois.append((t, pts([y + 1, y + 1, y + 2], [x + 1, x + 2, x + 1])))   # touches cell v
    img = np.full((T, H, W), 7, np.uint16)
    img[0, 0, 0] = 900
    return img, 1, rois


def case_empty(rng):
    return (rng.integers(0, 50, (2, 16, 16))).astype(np.uint16), 1, []


def run_case(name, img, C, rois, PolygonI):
    import tifffile
    from src.inference.analysis import AnalysisWorker
    from src.inference.result_export import ResultExportWorker
    csv = {}
    shapes = [[PolygonI(t, p)] for t, p in rois]
    image = FakeImage(img, C, shapes, f"{name}.tif", csv)
    CURRENT["image"] = image
    msgs = []
    out = {"img": img, "theT": np.array([t for t, _ in rois], np.int32),
           "points": np.array("\n".join(p for _, p in rois)), "shape": np.array(img.shape[:3], np.int64)}
    with tempfile.TemporaryDirectory() as d:
        d = pathlib.Path(d)
        aw = AnalysisWorker([1], d, "u", "p", "h", 4064, None)
        aw.text_output.connect(msgs.append)
        aw.analyze_data()
        ew = ResultExportWorker([1], d, "u", "p", "h", 4064, None)
        ew.text_output.connect(msgs.append)
        ew.export_data()
        res = d / "proj"
        out["messages"] = np.array("\n".join(msgs))
        if "text" in csv:
            out["csv"] = np.array(csv["text"].decode())
            assert (res / f"{name}_analysis.csv").read_bytes() == csv["text"]
            m = tifffile.imread(str(res / f"{name}_mask.tif"))
            out["mask"] = m.reshape(img.shape[:3])
            out["outlines"] = tifffile.imread(str(res / f"{name}_outlines.tif")).reshape(img.shape[:3])
            out["overlay"] = tifffile.imread(str(res / f"{name}_overlay.tif")).reshape(img.shape[:3] + (-1,))
        else:
            assert not any(res.glob("*")) if res.exists() else True
    print(name, {k: (v.shape, v.dtype) for k, v in out.items()}, msgs[-1:])
    np.savez_compressed(OUT / f"analysis_{name}.npz", **out)


def main():
    PolygonI = _install_placeholders()
    sys.path.remove(str(ROOT))                # `src` must be the reference's package, not this repository's shims
    for m in [m for m in sys.modules if m == "src" or m.startswith("src.")]:
        del sys.modules[m]
    sys.path.insert(0, "/root/reference")
    OUT.mkdir(parents=True, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(2026))
    for name, fn in (("mixed", case_mixed), ("rgb", case_rgb), ("wrap", case_wrap), ("empty", case_empty)):
        img, C, rois = fn(rng)
        run_case(name, img, C, rois, PolygonI)


if __name__ == "__main__":
    main()
