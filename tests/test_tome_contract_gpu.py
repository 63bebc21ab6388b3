"""GPU contract of mmt_tome_match and the ToMe merge kernels (csrc/tome.hip): the kernel chain that
ran, the boundaries of every chain, ties and NaN at scale, lane layouts, r == ta, strided views,
guards, refusals; merge fan-in above the LDS list, the merge limits, strided x / out.

Every match asserts mmt_tome_last_route() against tests/tome_ref.expected_route (the dispatch
restated in Python) and unm, src, dst and node_max bit for bit against oracle.tome.canon_match.
No tolerance anywhere. Metrics are `randn` (no ties) or tests/tome_ref.tie_metric (codebook rows:
ties across the r cut, fan-in >= 9, one NaN row in sample 1, all-NaN sample 2);
check_tie_properties runs on every oracle result of the latter, so data that stopped tying fails.
Oracle results are computed once per (data, r, flags) and shared."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import tome as O
from tests import tome_ref as R
from tests.seqnorm_ref import expected_rpt
from tests.test_tome_gpu import match_path  # noqa: F401  (the mfma / valu fixture)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
KINDS = pytest.mark.parametrize("kind", ["randn", "tie"])
SENT32, SENT8, G = 0x7FC00005, 0xA5, 64      # sentinels; guard words around every output
LAST_FUSED, LAST_BIG, LAST_BIG2 = R.form_boundaries(64)


def _mods():
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    return _C, K


# ------------------------------------------------------------------ data and oracle, shared
@functools.lru_cache(maxsize=None)
def _data(kind, n, t, heads, c, bf16):
    """(n, t, heads, c) fp32 values, exact in the dtype they will be stored in."""
    if kind == "tie":
        return R.tie_metric(n, t, heads, c)
    g = torch.Generator().manual_seed(7 + n * 1000 + t * 3 + c + heads)
    m = torch.randn((n, t, heads, c), generator=g)
    return (m.bfloat16().float() if bf16 else m).numpy()


@functools.lru_cache(maxsize=None)
def _oracle_cached(kind, n, t, heads, c, bf16, r, flags):
    out = O.canon_match(_data(kind, n, t, heads, c, bf16), r, flags)
    if kind == "tie":
        R.check_tie_properties(out[3], out[2], r)
    for a in out:
        a.setflags(write=False)
    return out


def _values(kind, n, t, heads, c, dtype):
    return _data(kind, n, t, heads, c, dtype == BF16 and kind != "tie")


def _oracle(kind, n, t, heads, c, dtype, r, flags):
    return _oracle_cached(kind, n, t, heads, c, dtype == BF16 and kind != "tie", r, flags)


def _strides(dm):
    return (dm.stride(0), dm.stride(1), dm.stride(2) if dm.dim() == 4 else 0)


def _assert_outputs(got, ref):
    unm, src, dst, nmax = (a.cpu().numpy() for a in got)
    np.testing.assert_array_equal(src, ref[1])
    np.testing.assert_array_equal(dst, ref[2])
    np.testing.assert_array_equal(unm, ref[0])
    np.testing.assert_array_equal(nmax.view(np.uint32), ref[3].view(np.uint32))


def _match(dev, kind, n, t, heads, c, r, flags, dtype, use_mfma=True, place=None):
    """One mmt_tome_match through the wrapper: the route against expected_route and the four
    outputs against the oracle. place: host (n, t, heads, c) tensor -> the device view to pass."""
    _C, K = _mods()
    host = torch.from_numpy(_values(kind, n, t, heads, c, dtype).copy()).to(dtype)
    if place is not None:
        dm = place(host)
    else:
        dm = host.to(dev) if heads > 1 else host[:, :, 0].to(dev)
    got = K.tome_match(dm, r, flags, return_node_max=True)
    route = _C.tome_last_route()
    torch.cuda.synchronize()
    exp = R.expected_route(n, t, c, dtype, _strides(dm), dm.data_ptr() % 16, use_mfma)
    assert route == exp, (hex(route), hex(exp))
    _assert_outputs(got, _oracle(kind, n, t, heads, c, dtype, r, flags))
    return route


def _form(route):
    return route & _mods()[0].TOME_ROUTE_FORM_MASK


# ------------------------------------------------------------------ form boundaries at c = 64
def test_boundaries_are_the_documented_ones():
    """include/mmt_api.h states t <= 513 / 1153 at c = 64; the helper derives them."""
    assert (LAST_FUSED, LAST_BIG, LAST_BIG2) == (513, 1153, 1089)


@DTYPES
@KINDS
@pytest.mark.parametrize("t,form", [(LAST_FUSED - 1, "FUSED"), (LAST_FUSED, "FUSED"),
                                    (LAST_FUSED + 1, "BIG_AG1"), (LAST_BIG, "BIG_AG1"),
                                    (LAST_BIG + 1, "TILED_MFMA")])
def test_form_boundaries_c64(dev, t, form, kind, dtype):
    _C, _ = _mods()
    route = _match(dev, kind, 2, t, 1, 64, 32, 0, dtype)
    assert route == _C.tome_route(getattr(_C, "TOME_ROUTE_" + form), 8,
                                  4 if form == "TILED_MFMA" else 0, dtype == BF16), hex(route)


@DTYPES
@KINDS
def test_two_a_tiles_per_workgroup(dev, kind, dtype):
    """(29, 514, 64): the smallest shape off the fused form with n * ceil(ta / 32) > 256."""
    _C, _ = _mods()
    t = LAST_FUSED + 1
    n = 256 // (((t + 1) // 2 + 31) // 32) + 1
    assert n == 29
    route = _match(dev, kind, n, t, 1, 64, 32, 0, dtype)
    assert route == _C.tome_route(_C.TOME_ROUTE_BIG_AG2, 8, 0, dtype == BF16), hex(route)


# ------------------------------------------------------------------ lane layouts
# t, c, heads, r -> (form, lpr, nbt) on the MFMA path; the VALU path is tiled VALU throughout
LAYOUTS = [(130, 24, 1, 16, ("FUSED", 4, 0)),      # LPR 4 with an idle lane, partial a and b tiles
           (64, 40, 3, 16, ("FUSED", 8, 0)),
           (258, 96, 1, 16, ("FUSED", 16, 0)),
           (64, 512, 1, 16, ("FUSED", 64, 0)),
           (130, 512, 1, 16, ("TILED_MFMA", 64, 1)),
           (300, 256, 2, 16, ("TILED_MFMA", 32, 3)),
           (300, 12, 1, 16, ("BIG_AG1", 0, 0)),        # c % 8 != 0, c % 4 == 0: scalar norm + big
           (301, 7, 1, 16, ("TILED_VALU", 0, 4)),      # odd c: VALU even when MFMA is requested
           (31, 6, 1, 12, ("TILED_MFMA", 0, 4))]       # scalar norm + tiled MFMA


@DTYPES
@KINDS
@pytest.mark.parametrize("t,c,heads,r,mfma_route", LAYOUTS)
def test_lane_layouts(dev, match_path, t, c, heads, r, mfma_route, kind, dtype):
    _C, _ = _mods()
    route = _match(dev, kind, 3, t, heads, c, r, 0, dtype, use_mfma=match_path)
    form, lpr, nbt = mfma_route
    if not match_path:
        form, nbt = "TILED_VALU", R.tiled_nbt(c)
    assert route == _C.tome_route(getattr(_C, "TOME_ROUTE_" + form), lpr, nbt, dtype == BF16), hex(route)


# ------------------------------------------------------------------ ties at scale
@DTYPES
@pytest.mark.parametrize("n,t,r,flags,form", [(3, 512, 32, 0, "FUSED"), (3, 1024, 32, 0, "BIG_AG1"),
                                              (3, 1000, 50, 3, "BIG_AG1"),
                                              (2, 2048, 64, 0, "TILED_MFMA"),
                                              (2, 2048, 64, 1, "TILED_MFMA")])
def test_ties_at_scale(dev, n, t, r, flags, form, dtype):
    """A tie across the r cut through the fused rank, rank8 over 4 blocks and rank with
    ta = 1024 (two rows per thread)."""
    _C, _ = _mods()
    route = _match(dev, "tie", n, t, 1, 64, r, flags, dtype)
    assert _form(route) == getattr(_C, "TOME_ROUTE_" + form), hex(route)


@contextlib.contextmanager
def _valu_path():
    """The VALU score path for the calls inside, the default again afterwards."""
    _, K = _mods()
    K.set_tome_match_path(False)
    try:
        yield
    finally:
        K.set_tome_match_path(True)


def test_ties_at_scale_valu(dev):
    """The tiled VALU score and the one-workgroup rank on the tie data of a b-resident shape."""
    _C, _ = _mods()
    with _valu_path():
        route = _match(dev, "tie", 3, 1000, 1, 64, 50, 3, F32, use_mfma=False)
    assert route == _C.tome_route(_C.TOME_ROUTE_TILED_VALU, 8, 4)


# ------------------------------------------------------------------ r == ta
def _merge_all(dev, x, s0, t, r, maps, size, flags, dtype, fused=True):
    """tome_merge_fwd, tome_pos_map, tome_merge_bwd (and the fused merge + sequence LayerNorm)
    on numpy maps (unm, src, dst) against the oracle, bit for bit."""
    _C, K = _mods()
    cu, cs, cd = maps
    n, L, D = x.shape
    tt = lambda a: torch.from_numpy(np.array(a)).to(dev)
    bf = lambda a: torch.from_numpy(a).bfloat16().float().numpy() if dtype == BF16 else a
    x = bf(x)
    xo_ref, so_ref = O.canon_merge_wavg(x[:, s0:s0 + t], size, cu, cs, cd, r, flags)
    xd, du, ds, dd, dsz = tt(x).to(dtype), tt(cu), tt(cs), tt(cd), tt(size)
    out, so, pos = K.tome_merge_fwd(xd, s0, t, r, du, ds, dd, size_in=dsz, flags=flags)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    np.testing.assert_array_equal(got[:, s0:s0 + t - r].view(np.uint32), bf(xo_ref).view(np.uint32))
    np.testing.assert_array_equal(got[:, :s0], x[:, :s0])
    np.testing.assert_array_equal(got[:, s0 + t - r:], x[:, s0 + t:])
    np.testing.assert_array_equal(so.cpu().numpy(), so_ref)
    if fused and dtype == F32:
        g = torch.Generator().manual_seed(D)
        gamma, beta = torch.randn(D, generator=g).to(dev), torch.randn(D, generator=g).to(dev)
        a_y, a_m, a_r = K.seqnorm_fwd(out, gamma, beta, 1e-6)
        b = K.tome_merge_seqnorm_fwd(xd, s0, t, r, du, ds, dd, gamma, beta, 1e-6, size_in=dsz,
                                     flags=flags)
        assert _C.norm_last_route() == _C.norm_route(_C.NORM_ROUTE_MERGE_SEQ_FWD, expected_rpt(L - r))
        for u, v in zip((out, so, a_y, a_m, a_r), (b[0], b[1], b[3], b[4], b[5])):
            assert torch.equal(u, v)
        if not flags & 8:
            assert torch.equal(pos, b[2])
    if flags & 8:
        return  # dropped src tokens have no merged row: pos_map only covers scattered merges
    pos_ref = O.canon_pos_map(cu, cs, cd, t, r, flags)
    np.testing.assert_array_equal(pos.cpu().numpy(), pos_ref)
    np.testing.assert_array_equal(K.tome_pos_map(du, ds, dd, t, r, flags).cpu().numpy(), pos_ref)
    rng = np.random.default_rng(L + D + r)
    g = bf(rng.standard_normal((n, L - r, D)).astype(np.float32))
    plain = bool(flags & 4)
    gi = K.tome_merge_bwd(tt(g).to(dtype), s0, t, r, pos, None if plain else dsz,
                          None if plain else so)
    torch.cuda.synchronize()
    gi = gi.float().cpu().numpy()
    gref = bf(O.canon_merge_bwd(g[:, s0:s0 + t - r], None if plain else size,
                                np.ones_like(so_ref) if plain else so_ref, pos_ref))
    np.testing.assert_array_equal(gi[:, s0:s0 + t].view(np.uint32), gref.view(np.uint32))
    np.testing.assert_array_equal(gi[:, :s0], g[:, :s0])
    np.testing.assert_array_equal(gi[:, s0 + t:], g[:, s0 + t - r:])


@DTYPES
@pytest.mark.parametrize("t,c,kind", [(8, 8, "randn"), (512, 64, "randn"), (512, 64, "tie")])
def test_every_a_token_merges(dev, t, c, kind, dtype):
    """r == ta: unm is empty (the wrapper) or NULL (the C call); match, merge forward, pos_map and
    merge backward."""
    _C, K = _mods()
    n, r = 2, t // 2
    _match(dev, kind, n, t, 1, c, r, 0, dtype)
    ref = _oracle(kind, n, t, 1, c, dtype, r, 0)
    assert ref[0].shape == (n, 0)
    m = torch.from_numpy(_values(kind, n, t, 1, c, dtype)[:, :, 0].copy()).to(dtype).to(dev)
    src = torch.full((n, r), -1, dtype=torch.int32, device=dev)
    dst, nmax = src.clone(), torch.zeros((n, r), device=dev)
    ws = torch.empty(_C.workspace_size(_C.WS_TOME_MATCH, n, t, c), dtype=torch.uint8, device=dev)
    _C.call("mmt_tome_match", m.data_ptr(), 1 if dtype == BF16 else 0, n, t, 1, c, t * c, c, 0, r,
            0, None, src.data_ptr(), dst.data_ptr(), nmax.data_ptr(), ws.data_ptr(), ws.numel(),
            _C.stream_ptr())
    assert _C.tome_last_route() == R.expected_route(n, t, c, dtype)
    torch.cuda.synchronize()
    _assert_outputs((torch.empty((n, 0), dtype=torch.int32), src, dst, nmax), ref)
    rng = np.random.default_rng(t)
    L, s0, D = t + 12, 4, 72
    x = rng.standard_normal((n, L, D)).astype(np.float32)
    size = rng.integers(1, 6, (n, t)).astype(np.float32)
    _merge_all(dev, x, s0, t, r, ref[:3], size, 0, dtype)
    # NULL unm straight into the merge and pos_map entry points
    pos = torch.empty((n, t), dtype=torch.int32, device=dev)
    _C.call("mmt_tome_pos_map", None, src.data_ptr(), dst.data_ptr(), n, t, r, 0, pos.data_ptr(),
            _C.stream_ptr())
    np.testing.assert_array_equal(pos.cpu().numpy(), O.canon_pos_map(*ref[:3], t, r, 0))
    xd = torch.from_numpy(x).to(dev)
    out = torch.empty((n, L - r, D), device=dev)
    so = torch.empty((n, t - r), device=dev)
    _C.call("mmt_tome_merge_wavg_fwd", xd.data_ptr(), 0, n, L, D, L * D, D, s0, t, r, 0, None, None,
            src.data_ptr(), dst.data_ptr(), out.data_ptr(), (L - r) * D, D, so.data_ptr(), None,
            _C.stream_ptr())
    xo_ref, so_ref = O.canon_merge_wavg(x[:, s0:s0 + t], None, *ref[:3], r, 0)
    np.testing.assert_array_equal(out[:, s0:s0 + t - r].cpu().numpy().view(np.uint32),
                                  xo_ref.view(np.uint32))
    np.testing.assert_array_equal(so.cpu().numpy(), so_ref)
    K.device_status()


# ------------------------------------------------------------------ views
def _qkv_slice(dev, pad_t=9, s0=5):
    def place(host):                       # (n, t, heads, c) -> buf (n, L, 3, heads, c)[:, s0:s0+t, 1]
        n, t, heads, c = host.shape
        buf = torch.full((n, t + pad_t, 3, heads, c), float("nan"), dtype=host.dtype, device=dev)
        v = buf[:, s0:s0 + t, 1]
        v.copy_(host)
        return v
    return place


def _padded_sn(dev, pad=16):
    def place(host):
        n, t, heads, c = host.shape
        buf = torch.full((n, t * heads * c + pad), float("nan"), dtype=host.dtype, device=dev)
        v = buf[:, :t * heads * c].view(n, t, heads, c)
        v.copy_(host)
        return v
    return place


def _base_off_one(dev):
    def place(host):
        buf = torch.full((host.numel() + 1,), float("nan"), dtype=host.dtype, device=dev)
        v = buf[1:].view(host.shape)
        v.copy_(host)
        return v
    return place


def _odd_st(dev):
    def place(host):                       # s_t = heads * c + 1 elements: no multiple of 16 B
        n, t, heads, c = host.shape
        assert heads == 1
        buf = torch.full((n, t, c + 1), float("nan"), dtype=host.dtype, device=dev)
        v = buf[:, :, :c].unsqueeze(2)
        v.copy_(host)
        return v
    return place


@DTYPES
@KINDS
@pytest.mark.parametrize("t,heads", [(130, 2), (600, 2), (130, 1), (600, 1)])
def test_views_route_and_match_as_contiguous(dev, t, heads, kind, dtype):
    """A key slice of a wider (n, L, 3, heads, c) buffer at token 5 and a padded s_n take the
    chain of the contiguous shape; a base offset by one element or an s_t that is no multiple of
    16 B take the scalar norm; the outputs are the contiguous ones (the same oracle result)."""
    _C, _ = _mods()
    n, c, r = 2, 64, 24
    base = _match(dev, kind, n, t, heads, c, r, 0, dtype)
    assert not base & _C.TOME_ROUTE_NORM_SCALAR
    for place in (_qkv_slice(dev), _padded_sn(dev)):
        assert _match(dev, kind, n, t, heads, c, r, 0, dtype, place=place) == base
    scalar = [_base_off_one(dev)] + ([_odd_st(dev)] if heads == 1 else [])
    for place in scalar:
        route = _match(dev, kind, n, t, heads, c, r, 0, dtype, place=place)
        assert route == _C.tome_route(_C.TOME_ROUTE_BIG_AG1, 0, 0, dtype == BF16), hex(route)


@DTYPES
def test_views_valu_path(dev, dtype):
    """The vector norm kernel itself (not the fused kernel's copy of it) on the strided slice."""
    _C, _ = _mods()
    with _valu_path():
        route = _match(dev, "tie", 2, 130, 2, 64, 24, 0, dtype, use_mfma=False, place=_qkv_slice(dev))
    assert route == _C.tome_route(_C.TOME_ROUTE_TILED_VALU, 8, 4, dtype == BF16)


# ------------------------------------------------------------------ guards and refusals
class _Raw:
    """A direct mmt_tome_match call whose outputs are interior slices of sentinel-filled buffers
    and whose workspace is exactly `ws_bytes` inside a larger sentinel buffer."""

    def __init__(self, dev, n, t, c, r, dtype=F32, kind="tie", heads=1):
        _C, _ = _mods()
        self.n, self.t, self.c, self.r, self.heads = n, t, c, r, heads
        self.ta = ta = (t + 1) // 2
        self.dtype = dtype
        if kind is None:
            self.m = torch.zeros((n, t, heads, c), dtype=dtype, device=dev)
        else:
            self.m = torch.from_numpy(_values(kind, n, t, heads, c, dtype).copy()).to(dtype).to(dev)
        self.outs = [torch.full((G + n * ta + G,), SENT32, dtype=torch.int32, device=dev)
                     for _ in range(4)]                      # unm, src, dst, node_max
        self.need = _C.workspace_size(_C.WS_TOME_MATCH, n, t, c)
        self.ws = torch.full((256 + self.need + 256,), SENT8, dtype=torch.uint8, device=dev)
        assert self.ws.data_ptr() % 16 == 0
        self.before = [o.clone() for o in self.outs]

    def call(self, r=None, flags=0, dtype_code=None, ws_off=256, ws_bytes=None):
        _C, _ = _mods()
        t, c, heads = self.t, self.c, self.heads
        code = (1 if self.dtype == BF16 else 0) if dtype_code is None else dtype_code
        p = [o.data_ptr() + 4 * G for o in self.outs]
        _C.call("mmt_tome_match", self.m.data_ptr(), code, self.n, t, heads, c, t * heads * c,
                heads * c, c if heads > 1 else 0, self.r if r is None else r, flags, *p,
                self.ws.data_ptr() + ws_off, self.need if ws_bytes is None else ws_bytes,
                _C.stream_ptr())
        torch.cuda.synchronize()

    def sizes(self):
        return (self.n * (self.ta - self.r), self.n * self.r, self.n * self.r, self.n * self.ta)

    def result(self):
        n, r, ta = self.n, self.r, self.ta
        shapes = ((n, ta - r), (n, r), (n, r), (n, ta))
        v = [o[G:G + k].view(s) for o, k, s in zip(self.outs, self.sizes(), shapes)]
        v[3] = v[3].view(torch.float32)
        return v

    def guards_intact(self):
        ok = all(torch.equal(o[:G], b[:G]) and torch.equal(o[G + k:], b[G + k:])
                 for o, b, k in zip(self.outs, self.before, self.sizes()))
        return ok and bool((self.ws[:256] == SENT8).all()) and bool((self.ws[256 + self.need:] == SENT8).all())

    def untouched(self):
        return all(torch.equal(o, b) for o, b in zip(self.outs, self.before)) and bool(
            (self.ws == SENT8).all())


# one shape per chain: (n, t, c, heads, r, use_mfma) -> form
GUARD_SHAPES = [(3, 130, 24, 1, 16, True, "FUSED"), (2, 514, 64, 1, 32, True, "BIG_AG1"),
                (29, 514, 64, 1, 32, True, "BIG_AG2"), (3, 130, 512, 1, 16, True, "TILED_MFMA"),
                (3, 301, 7, 1, 16, True, "TILED_VALU"), (3, 300, 12, 1, 16, True, "BIG_AG1"),
                (3, 130, 24, 1, 16, False, "TILED_VALU")]


@DTYPES
@pytest.mark.parametrize("n,t,c,heads,r,use_mfma,form", GUARD_SHAPES)
def test_guards(dev, n, t, c, heads, r, use_mfma, form, dtype):
    _C, K = _mods()
    raw = _Raw(dev, n, t, c, r, dtype)
    m0 = raw.m.clone()
    with contextlib.nullcontext() if use_mfma else _valu_path():
        raw.call()
    route = _C.tome_last_route()
    assert route == R.expected_route(n, t, c, dtype, use_mfma=use_mfma), hex(route)
    assert _form(route) == getattr(_C, "TOME_ROUTE_" + form)
    assert raw.guards_intact() and torch.equal(raw.m, m0)
    _assert_outputs(raw.result(), _oracle("tie", n, t, heads, c, dtype, r, 0))


REFUSALS = [("t_2049", dict(t=2049, c=8), {}), ("c_513", dict(t=8, c=513), {}),
            ("r_0", {}, dict(r=0)), ("r_over_flags0", {}, dict(r=33)),
            ("r_over_flags1", {}, dict(r=32, flags=1)), ("r_over_flags2", {}, dict(r=32, flags=2)),
            ("r_over_flags3", {}, dict(r=32, flags=3)), ("ws_one_byte_short", {}, dict(ws_bytes=-1)),
            ("ws_misaligned", {}, dict(ws_off=260)), ("bad_dtype", {}, dict(dtype_code=2))]


@pytest.mark.parametrize("name,shape,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(dev, name, shape, kw):
    """Each gives MMTError, leaves tome_last_route() at NONE and touches neither the outputs nor
    the workspace. (t = 64, c = 16: r = 32 = ta is legal without protected tokens, one too many
    with any.) A valid call first, so that NONE is the refusal's doing."""
    _C, _ = _mods()
    ok = _Raw(dev, 2, 64, 16, 32)
    ok.call()
    assert _C.tome_last_route() == R.expected_route(2, 64, 16, F32)
    _assert_outputs(ok.result(), _oracle("tie", 2, 64, 1, 16, F32, 32, 0))
    raw = _Raw(dev, 1 if shape else 2, shape.get("t", 64), shape.get("c", 16), 2 if shape else 32,
               kind=None if shape else "tie")
    kw = dict(kw)
    if kw.get("ws_bytes") == -1:
        kw["ws_bytes"] = raw.need - 1
    with pytest.raises(_C.MMTError):
        raw.call(**kw)
    assert _C.tome_last_route() == _C.TOME_ROUTE_NONE
    assert raw.untouched()


# ------------------------------------------------------------------ merge: fan-in, limits, strides
def _hand_maps(n, t, r, dst_row, seed):
    """dst as given for every sample; src and unm a shuffled partition of the a half."""
    ta = (t + 1) // 2
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(ta) for _ in range(n)]).astype(np.int32)
    dst = np.tile(np.asarray(dst_row, np.int32), (n, 1))
    return perm[:, r:].copy(), perm[:, :r].copy(), dst


@functools.lru_cache(maxsize=None)
def _fan_in_maps(name):
    """(n, L, s0, t, D, r, (unm, src, dst)): fan-in of exactly 8 and 9 (the LDS list holds 8), and
    the maps of tie metrics. L - r = 64 and 84: register-resident forms of the fused merge +
    LayerNorm; 422: its two-pass form (L - r in (320, 512])."""
    if name == "hand":
        n, L, s0, t, D, r = 2, 84, 5, 64, 72, 20
        maps = _hand_maps(n, t, r, [0] * 8 + [1] * 9 + [2] * 3, 1)
    else:
        n, L, s0, t, D, r = {"tie130": (2, 144, 6, 130, 72, 60), "tie512": (2, 522, 6, 512, 72, 100)}[name]
        out = O.canon_match(R.tie_metric(n, t, 1, 64), r, 0)
        R.check_tie_properties(out[3], out[2], r)
        maps = out[:3]
    fan = np.bincount(maps[2][0])
    assert fan.max() >= 9 and (name != "hand" or sorted(fan.tolist()) == [3, 8, 9])
    return n, L, s0, t, D, r, maps


@DTYPES
@pytest.mark.parametrize("flags", [0, 2, 4, 8, 12])
@pytest.mark.parametrize("name", ["hand", "tie130", "tie512"])
def test_merge_fan_in_above_the_list(dev, name, flags, dtype):
    n, L, s0, t, D, r, maps = _fan_in_maps(name)
    rng = np.random.default_rng(L + flags)
    x = rng.standard_normal((n, L, D)).astype(np.float32)
    size = rng.integers(1, 6, (n, t)).astype(np.float32)
    _merge_all(dev, x, s0, t, r, maps, size, flags, dtype)
    _mods()[1].device_status()


@DTYPES
@pytest.mark.parametrize("t,r", [(2048, 512), (2048, 1), (2050, 1)])
def test_merge_limits_run(dev, t, r, dtype):
    """r = 512 and nu = ta - r = 1023 / 1024, the sizes of the kernels' LDS maps, at D = 8."""
    n, D = 1, 8
    rng = np.random.default_rng(t + r)
    cu, cs, _ = _hand_maps(n, t, r, [0] * r, t)
    cd = rng.integers(0, t // 2, (n, r)).astype(np.int32)
    x = rng.standard_normal((n, t, D)).astype(np.float32)
    size = rng.integers(1, 6, (n, t)).astype(np.float32)
    _merge_all(dev, x, 0, t, r, (cu, cs, cd), size, 0, dtype, fused=False)
    _mods()[1].device_status()


@pytest.mark.parametrize("t,r", [(2052, 1), (2048, 513)])
def test_merge_limits_refused(dev, t, r):
    _C, K = _mods()
    n, D = 1, 8
    cu, cs, cd = (torch.from_numpy(a).to(dev) for a in _hand_maps(n, t, r, [0] * r, 3))
    x = torch.zeros((n, t, D), device=dev)
    out = torch.full((n, t - r, D), 7.0, device=dev)
    with pytest.raises(_C.MMTError):
        K.tome_merge_fwd(x, 0, t, r, cu, cs, cd, out=out)
    with pytest.raises(_C.MMTError):
        K.tome_pos_map(cu, cs, cd, t, r)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@DTYPES
def test_merge_strided_x_and_out(dev, dtype):
    """x and out as slices of wider buffers (row stride above D, column offset 8): the result of
    the contiguous run, nothing outside the out view written; D or a stride that is no multiple
    of 16 B is refused."""
    _C, K = _mods()
    n, L, s0, t, D, r, maps = _fan_in_maps("hand")
    du, ds, dd = (torch.from_numpy(a).to(dev) for a in maps)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, L, D), generator=g).to(dtype).to(dev)
    size = torch.randint(1, 6, (n, t), generator=g).float().to(dev)
    ref, so_ref, pos_ref = K.tome_merge_fwd(x, s0, t, r, du, ds, dd, size_in=size)
    xbuf = torch.full((n, L + 8, D + 16), float("nan"), dtype=dtype, device=dev)
    xv = xbuf[:, 4:4 + L, 8:8 + D]
    xv.copy_(x)
    it = torch.int16 if dtype == BF16 else torch.int32
    obuf = torch.full((n, L - r + 8, D + 24), 0x7FC5 if dtype == BF16 else SENT32, dtype=it, device=dev)
    before = obuf.clone()
    ov = obuf.view(dtype)[:, 4:4 + L - r, 8:8 + D]
    out, so, pos = K.tome_merge_fwd(xv, s0, t, r, du, ds, dd, size_in=size, out=ov)
    torch.cuda.synchronize()
    assert out.data_ptr() == ov.data_ptr()
    assert torch.equal(ov.contiguous().view(it), ref.view(it))
    assert torch.equal(so, so_ref) and torch.equal(pos, pos_ref)
    now = obuf.clone()
    now[:, 4:4 + L - r, 8:8 + D] = before[:, 4:4 + L - r, 8:8 + D]
    assert torch.equal(now, before)
    # refusals: an odd row stride; a D that is no multiple of the 16-B vector
    odd = torch.zeros((n, L, D + 1), dtype=dtype, device=dev)[:, :, :D]
    with pytest.raises(_C.MMTError):
        K.tome_merge_fwd(odd, s0, t, r, du, ds, dd)
    with pytest.raises(_C.MMTError):
        K.tome_merge_fwd(x, s0, t, r, du, ds, dd, out=torch.zeros((n, L - r, D + 1), dtype=dtype,
                                                                 device=dev)[:, :, :D])
    Dbad = D - 4 if dtype == BF16 else D - 2
    with pytest.raises(_C.MMTError):
        K.tome_merge_fwd(x[:, :, :Dbad].contiguous(), s0, t, r, du, ds, dd)
    gi = torch.zeros((n, L - r, Dbad), dtype=dtype, device=dev)
    with pytest.raises(_C.MMTError):
        K.tome_merge_bwd(gi, s0, t, r, pos_ref, size, so_ref)
    K.device_status()
