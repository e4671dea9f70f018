"""Host (no GPU): what microbeseg_amd/engine.py says about a layer's launches and about bf16 tensor storage.  The library is
loaded; the dispatch queries launch nothing and need no device.

* bf16_storage_ok on a fixed grid of networks x batch x size x (eval | training) against the answers recorded before the
  launches were described in one place (tests/golden/bf16_storage_grid.json), and the documented guarantees directly;
* engine.layer_launches against the independent geometry of the convolution tables (conv_table.geom), the pack_weight
  recipes against the tuples written out here;
* the storage question and the launches share one cache of the library's answers."""
import pytest

import conv_table as CT
from helpers import storage_grid


@pytest.fixture(scope="module")
def E():
    from microbeseg_amd import engine
    return engine


@pytest.fixture(scope="module")
def grid():
    return storage_grid()


def _net(cfg):
    from microbeseg_amd.utils.unets import DUNet, UNet
    return (DUNet if cfg["unet"] == "DU" else UNet)(ch_in=cfg["ch_in"], pool_method=cfg["pool"], filters=tuple(cfg["filters"]))


def test_storage_answers_are_the_recorded_ones(E, grid):
    nets, table = grid
    assert len(table) == 600 and sum(table.values()) == 190
    wrong = []
    for name, cfg in nets.items():
        spec = _net(cfg)._spec
        for (nm, N, H, training), want in table.items():
            if nm == name and E.bf16_storage_ok(spec, N, cfg["ch_in"], H, H, training) != want:
                wrong.append((name, N, H, training, want))
    assert not wrong, wrong


def test_documented_storage_guarantees(E, grid):
    nets, table = grid
    NS, HS = sorted({k[1] for k in table}), sorted({k[2] for k in table})
    du = _net(nets["DU_64_1024"])._spec
    for N in NS:
        assert E.bf16_storage_ok(du, N, 1, 256, 256, True), N
        assert E.bf16_storage_ok(du, N, 1, 320, 320, True) == (N % 8 == 0), N
    for name, cfg in nets.items():
        spec = _net(cfg)._spec
        never = cfg["pool"] == "max" or any(f % 8 for f in cfg["filters"])
        for N in NS:
            for H in HS:
                for training in (False, True):
                    if never or (training and cfg["ch_in"] != 1):
                        assert not E.bf16_storage_ok(spec, N, cfg["ch_in"], H, H, training), (name, N, H, training)


IGEMM_FIELDS = ("Hi", "Wi", "Ho", "Wo", "stride", "pad", "mode", "Ngemm", "epi", "Cq", "morder")
WGRAD_FIELDS = ("Hp", "Wp", "Hq", "Wq", "stride", "pad")


def _same(kw, r, fields):
    g = CT.geom(r)
    assert kw["NB"] == r.N and kw["KH"] == kw["KW"] == g["K"], (r.op, kw)
    for f in fields:
        assert kw.get(f, 0) == g[f], (r.op, f, kw.get(f, 0), g[f])       # (EPI_PLAIN, MORDER_LINEAR, Cq default to 0)


@pytest.mark.parametrize("N,Ci,Co,H", [(2, 64, 128, 16), (3, 128, 64, 20)])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_launches_match_the_table_geometry(E, N, Ci, Co, H, stride):
    L = E.layer_launches("conv" if stride == 1 else "pool", (Ci,), Co, N, H, H)
    Ho = CT.CR.out_size(H, stride)
    assert L.out == (Ho, Ho)
    _same(L.fwd, CT.row("f", "conv", N, [Ci], Co, H, H, None, stride=stride), IGEMM_FIELDS)
    _same(L.dgrad, CT.row("d", "dgrad", N, [Co], Ci, Ho, Ho, None, stride=stride), IGEMM_FIELDS)
    _same(L.wgrad, CT.row("w", "wgrad3", N, [Ci], Co, Ho, Ho, None, stride=stride), WGRAD_FIELDS)
    assert L.fwd["ld0"] == Co and L.dgrad["ld0"] == Ci and "split" not in L.dgrad
    dz, xs = object(), [object()]
    assert E._wgrad_operands(L, dz, xs) == (dz, xs)                           # P = dz (Co channels), Q = the input
    assert L.pack_fwd == (9, Co, Ci, 1, Ci * 9, 9, False)                 # the tuples of the call sites before the refactor
    assert L.pack_dgrad == (9, Ci, Co, 1, 9, Ci * 9, False)


@pytest.mark.parametrize("N,Ci,Co,H", [(2, 64, 128, 16), (3, 128, 64, 20)])
def test_convtranspose_launches_match_the_table_geometry(E, N, Ci, Co, H):
    L = E.layer_launches("up", (Ci,), Co, N, H, H)
    assert L.out == (2 * H, 2 * H)
    _same(L.fwd, CT.row("f", "convT", N, [Ci], Co, H, H, None), IGEMM_FIELDS)
    _same(L.dgrad, CT.row("d", "convT_dgrad", N, [Co], Ci, 2 * H, 2 * H, None), IGEMM_FIELDS)
    _same(L.wgrad, CT.row("w", "wgrad2", N, [Co], Ci, H, H, None), WGRAD_FIELDS)
    assert L.fwd["ld0"] == Co and L.dgrad["ld0"] == Ci
    dz, xs = object(), [object()]
    assert E._wgrad_operands(L, dz, xs) == (xs[0], [dz])                      # P = the input (Ci channels), Q = dz
    assert L.pack_fwd == (4, Co, Ci, 1, 4, Co * 4, True)
    assert L.pack_dgrad == (4, Ci, Co, 1, Co * 4, 4, False)


def test_concat_layer_splits_its_data_gradient(E):
    L = E.layer_launches("conv", (64, 64), 64, 2, 16, 16)
    _same(L.fwd, CT.row("f", "conv", 2, [64, 64], 64, 16, 16, None), IGEMM_FIELDS)
    _same(L.dgrad, CT.row("d", "dgrad", 2, [64], 128, 16, 16, None), IGEMM_FIELDS)
    assert L.dgrad["split"] == L.dgrad["ld0"] == 64 and L.dgrad["ld1"] == 64
    assert L.pack_fwd == (9, 64, 128, 1, 128 * 9, 9, False) and L.pack_dgrad == (9, 128, 64, 1, 9, 128 * 9, False)


def test_first_layer_rule(E):
    """the conditions as they stood at the three places that held them: 256 % (cout // 8) for the raw-frame kernel,
    256 % (cout // 4) for the VALU kernels"""
    for cin in (1, 2, 3, 4, 5):
        for cout in (4, 8, 12, 16, 24, 48, 64, 96, 128, 256, 512):
            valu = 1 <= cin <= 4 and cout % 4 == 0 and cout <= 256 and 256 % (cout // 4) == 0
            for raw in (False, True):
                for tape in (False, True):
                    f = E.first_layer(cin, cout, raw=raw, tape=tape)
                    fused = raw and not tape and cin == 1 and cout % 8 == 0 and cout <= 256 and 256 % (cout // 8) == 0
                    assert f.fwd == ("raw" if fused else "valu" if valu else "igemm"), (cin, cout, raw, tape)
                    assert f.bwd == ("first_wgrad" if cin == 1 and valu else "wgrad")
                    assert f.bf16_storage == (valu and cout % 8 == 0 and not (tape and cin != 1))


def test_storage_question_and_launches_share_one_cache(E, grid, monkeypatch):
    nets, _ = grid
    asked = []
    query = E._query
    monkeypatch.setattr(E, "_query", lambda fn, p: (asked.append(1), query(fn, p))[1])
    net = _net(nets["DU_64_128"])
    assert E.bf16_storage_ok(net._spec, 2, 1, 64, 64, True)
    first = len(asked)
    assert E.bf16_storage_ok(net._spec, 2, 1, 64, 64, True) and len(asked) == first
    # a second network of the same shapes: its own memo is empty, every launch is answered from the launches' cache
    assert E.bf16_storage_ok(_net(nets["DU_64_128"])._spec, 2, 1, 64, 64, True) and len(asked) == first
    # ... which is the one E.igemm / E.wgrad ask: the descriptor of a real launch of this network is in it
    t16, L = E._PH[E.ST_BF16], E.layer_launches("conv", (64,), 64, 2, 64, 64)
    src = E.Node(t16, 2, 64, 64, 64)
    src.act, src.scale, src.shift = E.ACT["relu"], E._PH[E.ST_F32], E._PH[E.ST_F32]
    npad, kpad = E._pack_dims(*L.pack_fwd)
    assert E._igemm_bf16_ok(E._igemm_desc([src.src()], kpad, npad, E._PH[E.ST_F32], t16, None, **L.fwd))
    assert len(asked) == first
