"""GPU: the pad-mask kernels (csrc/padmask.hip; include/mmt_api.h "observation pad masks")
against the numpy restatement tests/pad_mask_ref.py, all exact: every value is 0, M, pe[l], a
copied pixel or one fp32 add that numpy reproduces. Set layouts: [0,5) [5,12) [12,15) [15,19) (L 19, padded 64) and
[0,70) [70,96) [96,100) (L 100, padded 128: two 64-blocks of bias rows, seven 16-row blocks of
sequence rows with a tail of 4)."""
import numpy as np
import pytest
import torch

from tests import pad_mask_ref as R

pytestmark = pytest.mark.gpu

B = 3
LAYOUTS = {
    "L19": ([0, 5, 12, 15], [5, 7, 3, 4],
            np.array([[1, 0, 1, 1], [0, 1, 0, 1], [1, 1, 1, 1]], bool), 0b1000),
    "L100": ([0, 70, 96], [70, 26, 4],
             np.array([[0, 1, 1], [1, 0, 1], [1, 1, 1]], bool), 0b100),
}


def _text_mask(T, seed=0):
    """Instruction lengths 3, T, 1 of T."""
    tm = np.zeros((B, T), bool)
    for b, n in enumerate((3, T, 1)):
        tm[b, :n] = True
    return tm


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(dev, key, text):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    starts, lens, sm, rbits = LAYOUTS[key]
    tm = _text_mask(lens[0]) if text else None
    words = K.pad_mask_pack(torch.from_numpy(sm).to(dev), rbits)
    masked = R.masked_rows(starts, lens, B, sm, tm, 0, rbits)
    t_dev = None if tm is None else torch.from_numpy(tm).to(dev)
    return K, starts, lens, words, t_dev, masked


def test_pack(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    rng = np.random.default_rng(0)
    for n, Bn in ((1, 1), (4, 3), (7, 300), (16, 257)):
        sm = rng.random((Bn, n)) < 0.6
        rbits = 1 << (n - 1)
        sm[:, n - 1] = True
        words = K.pad_mask_pack(torch.from_numpy(sm).to(dev), rbits)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(words.cpu().numpy().view(np.uint32), R.pack(sm, rbits))
    K.device_status()


def test_pack_reports_an_absent_readout_set(dev):
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    K.device_status()   # clean before
    sm = np.array([[1, 1, 1, 1], [1, 0, 1, 0], [1, 1, 1, 1]], bool)
    words = K.pad_mask_pack(torch.from_numpy(sm).to(dev), 0b1000)
    with pytest.raises(_C.MMTError, match="MMT_FAULT_PAD_MASK"):
        K.device_status()
    # the set is treated as present: the packed word has its bit
    assert words.cpu().numpy().view(np.uint32).tolist() == [0b1111, 0b1101, 0b1111]
    K.device_status()   # the status word was cleared


@pytest.mark.parametrize("key", list(LAYOUTS))
@pytest.mark.parametrize("text", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_bias_rows(dev, key, text, view):
    """accumulate 0 and 1, with and without a text mask on set 0, into a contiguous buffer and
    through a view with a larger row stride (whose columns past the view keep their canary)."""
    K, starts, lens, words, tm, masked = _case(dev, key, text)
    L = sum(lens)
    lp = K.attn_lp(L)
    assert lp == {19: 64, 100: 128}[L]
    width = lp + 12 if view else lp
    buf = torch.full((B, width), 7.0, device=dev)
    kb = K.pad_mask_bias(B, L, (starts, lens), words, tm, out=buf[:, :lp])
    assert kb.data_ptr() == buf.data_ptr() and kb.stride(0) == width
    torch.cuda.synchronize()
    want = R.bias_rows(masked, lp)
    np.testing.assert_array_equal(_bits(buf[:, :lp]), _bits(want))
    assert (buf[:, :lp][:, L:] == 0).all()                       # the padding is written 0
    assert (buf[:, lp:] == 7.0).all()
    assert masked.any() and not masked.all()
    if not view:   # the allocating form gives the same rows
        assert torch.equal(K.pad_mask_bias(B, L, (starts, lens), words, tm), buf)
    # accumulate: random finite floats on [0, L), NaN in the padding, untouched but for one add
    g = torch.Generator().manual_seed(L)
    base = torch.full((B, width), float("nan"))
    base[:, :L] = torch.randn((B, L), generator=g) * 3
    acc = base.clone().to(dev)
    K.pad_mask_bias(B, L, K.SetTable(starts, lens, [1] * len(lens)), words, tm, out=acc[:, :lp],
                    accumulate=True)
    torch.cuda.synchronize()
    want = R.bias_rows(masked, width, base.numpy())
    np.testing.assert_array_equal(_bits(acc), _bits(want))
    assert np.isnan(acc.cpu().numpy()[:, L:]).all()
    K.device_status()


def test_bias_text_mask_alone_and_on_a_later_set(dev):
    """No set mask at all (words NULL), and the text set second in the sequence."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    starts, lens = [0, 5, 12, 15], [5, 7, 3, 4]
    tm = _text_mask(7)
    kb = K.pad_mask_bias(B, 19, (starts, lens), None, torch.from_numpy(tm).to(dev), text_set=1)
    torch.cuda.synchronize()
    masked = R.masked_rows(starts, lens, B, None, tm, 1)
    np.testing.assert_array_equal(_bits(kb), _bits(R.bias_rows(masked, 64)))


@pytest.mark.parametrize("key", list(LAYOUTS))
@pytest.mark.parametrize("D", [8, 48])
@pytest.mark.parametrize("text", [False, True])
def test_rows_fwd_and_bwd(dev, key, D, text):
    """x0[b, l] = pe[l] / dx0[b, l] = 0 on the masked rows; the others bit-unchanged (NaN rows
    among them would show a rewrite through arithmetic); a canary behind the buffer intact."""
    K, starts, lens, words, tm, masked = _case(dev, key, text)
    L = sum(lens)
    g = torch.Generator().manual_seed(L + D)
    x = torch.randn((B, L, D), generator=g)
    x[2, L - 1] = float("nan")                   # a present row: must come back bit-equal
    assert not masked[2, L - 1]
    pe = torch.randn((L, D), generator=g)
    n = B * L * D
    for which in ("fwd", "bwd"):
        buf = torch.full((n + 64,), -3.0, device=dev)
        buf[:n] = x.view(-1).to(dev)
        xv = buf[:n].view(B, L, D)
        if which == "fwd":
            K.pad_mask_rows_fwd(xv, pe.to(dev), (starts, lens), words, tm)
            want = R.rows_fwd(x.numpy(), pe.numpy(), masked)
        else:
            K.pad_mask_rows_bwd(xv, (starts, lens), words, tm)
            want = R.rows_bwd(x.numpy(), masked)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(xv), _bits(want))
        np.testing.assert_array_equal(_bits(xv)[~masked], _bits(x)[~masked])
        assert (buf[n:] == -3.0).all()
    K.device_status()


def test_rows_through_a_strided_view(dev):
    """Row stride above D and sample stride above L rows: the gaps keep their canary."""
    K, starts, lens, words, tm, masked = _case(dev, "L19", True)
    L, D, xs_t = 19, 8, 12
    xs_b = L * xs_t + 8
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, L, D), generator=g)
    pe = torch.randn((L, D), generator=g)
    buf = torch.full((B * xs_b,), -3.0, device=dev)
    xv = buf.as_strided((B, L, D), (xs_b, xs_t, 1))
    xv.copy_(x.to(dev))
    K.pad_mask_rows_fwd(xv, pe.to(dev), (starts, lens), words, tm)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(xv), _bits(R.rows_fwd(x.numpy(), pe.numpy(), masked)))
    gaps = torch.ones(B * xs_b, dtype=torch.bool, device=dev)
    gaps.as_strided((B, L, D), (xs_b, xs_t, 1)).fill_(False)
    assert (buf[gaps] == -3.0).all() and int(gaps.sum()) == B * xs_b - B * L * D


@pytest.mark.parametrize("dtype,shape", [(torch.uint8, (5, 2, 8, 8, 3)),       # 192 B: one tail block
                                         (torch.uint8, (3, 3, 64, 64, 3)),    # 12 vectors a thread
                                         (torch.float32, (2, 2, 40, 40, 3))])  # 1200 vectors: a tail
def test_images_of_absent_cameras_are_zeroed_in_a_copy(dev, dtype, shape):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    Bn, I = shape[:2]
    rng = np.random.default_rng(Bn + I)
    n_sets = I + 2                                     # text | cameras | readout
    image_sets = list(range(1, I + 1))
    sm = rng.random((Bn, n_sets)) < 0.5
    sm[:, -1] = True
    sm[0, 1], sm[1, 1] = False, True                   # both cases present
    img = torch.from_numpy(rng.integers(1, 255, shape)).to(dtype)
    n = img.numel()
    buf = torch.full((n + 64,), 7, dtype=dtype, device=dev)
    out = buf[:n].view(shape)
    src = img.to(dev)
    words = K.pad_mask_pack(torch.from_numpy(sm).to(dev), 1 << (n_sets - 1))
    got = K.pad_mask_images(src, words, image_sets, n_sets, out=out)
    torch.cuda.synchronize()
    want = img.clone()
    for b in range(Bn):
        for i, s_ in enumerate(image_sets):
            if not sm[b, s_]:
                want[b, i] = 0
    assert got.data_ptr() == buf.data_ptr() and torch.equal(out.cpu(), want)
    assert torch.equal(src.cpu(), img) and (buf[n:] == 7).all()      # the input and the canary
    assert torch.equal(K.pad_mask_images(src, words, image_sets, n_sets).cpu(), want)
    with pytest.raises(ValueError):
        K.pad_mask_images(src, words, image_sets[:-1], n_sets)
    from multi_modal_transformers_tokenmerge_amd import _C
    with pytest.raises(_C.MMTError, match="mmt_pad_mask_images"):
        K.pad_mask_images(src, words, image_sets, n_sets, out=src)   # in place is refused
    with pytest.raises(_C.MMTError, match="mmt_pad_mask_images"):
        K.pad_mask_images(src, words, [n_sets] * I, n_sets)          # a set past the table
    assert torch.equal(src.cpu(), img)
    K.device_status()


def test_guards_return_before_a_launch(dev):
    """Every MMT_ERR_INVALID guard with real device buffers: MMTError, the outputs untouched."""
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    starts, lens, sm, rbits = LAYOUTS["L19"]
    L, D, lp = 19, 8, 64
    words = K.pad_mask_pack(torch.from_numpy(sm).to(dev), rbits)
    tm = torch.from_numpy(_text_mask(5)).to(dev)
    kb = torch.full((B, lp + 8), 7.0, device=dev)
    x = torch.full((B, L + 1, D + 4), 7.0, device=dev)
    pe = torch.zeros((L, D), device=dev)
    arr = lambda v: (_C.ctypes.c_int32 * len(v))(*v)   # noqa: E731
    S = _C.stream_ptr()

    def bias(words_=words, L_=L, n=4, st=starts, ln=lens, text=None, ts=0, T=0, kb_=None,
             stride=lp + 8, off=0):
        p = kb.data_ptr() + off if kb_ is None else kb_
        return _C.call("mmt_pad_mask_bias", _C.ptr(words_), B, L_, n, arr(st), arr(ln),
                       _C.ptr(text), ts, T, p, stride, 0, S)

    def rows(which="fwd", words_=words, D_=D, n=4, st=starts, ln=lens, text=None, ts=0, T=0,
             pe_=pe, off=0, xs_b=(L + 1) * (D + 4), xs_t=D + 4):
        head = (_C.ptr(words_), B, L, D_, n, arr(st), arr(ln), _C.ptr(text), ts, T)
        tail = (x.data_ptr() + off, xs_b, xs_t, S)
        if which == "fwd":
            return _C.call("mmt_pad_mask_rows_fwd", *head, _C.ptr(pe_), *tail)
        return _C.call("mmt_pad_mask_rows_bwd", *head, *tail)

    bad = [
        lambda: bias(words_=None), lambda: bias(n=0), lambda: bias(n=17),
        lambda: bias(st=[0, 6, 12, 15]), lambda: bias(ln=[5, 7, 3, 5]), lambda: bias(L_=20),
        lambda: bias(stride=60), lambda: bias(stride=lp + 2), lambda: bias(off=4),
        lambda: bias(kb_=0), lambda: bias(text=tm, T=4), lambda: bias(text=tm, T=5, ts=4),
        lambda: bias(text=tm, T=5, ts=1),
        lambda: rows(words_=None), lambda: rows(n=17), lambda: rows(D_=6), lambda: rows(off=4),
        lambda: rows(pe_=None), lambda: rows(xs_t=4), lambda: rows(xs_t=D + 2),
        lambda: rows(xs_b=(L + 1) * (D + 4) + 2), lambda: rows(xs_b=8), lambda: rows(text=tm, T=7),
        lambda: rows(st=[0, 5, 13, 15]),
        lambda: rows("bwd", words_=None), lambda: rows("bwd", D_=6), lambda: rows("bwd", off=8),
        lambda: rows("bwd", xs_t=4), lambda: rows("bwd", ln=[5, 7, 3, 3]),
        lambda: rows("bwd", text=tm, T=5, ts=-1),
        lambda: _C.call("mmt_pad_mask_pack", None, B, 4, rbits, words.data_ptr(), S),
        lambda: _C.call("mmt_pad_mask_pack", tm.data_ptr(), B, 17, 0, words.data_ptr(), S),
        lambda: _C.call("mmt_pad_mask_pack", tm.data_ptr(), B, 4, 0b10000, words.data_ptr(), S),
    ]
    before = words.clone()
    for i, call in enumerate(bad):
        with pytest.raises(_C.MMTError, match="mmt_pad_mask_"):
            call()
            pytest.fail(f"guard {i} let the call through")
    torch.cuda.synchronize()
    assert (kb == 7.0).all() and (x == 7.0).all() and torch.equal(words, before)
    # the good forms of the same helpers do launch
    bias(text=tm, T=5)
    rows(text=tm, T=5)
    rows("bwd")
    torch.cuda.synchronize()
    assert not (kb == 7.0).all() and not (x == 7.0).all()
    K.device_status()
    # the wrappers' own host checks
    with pytest.raises(ValueError):
        K.pad_mask_bias(B, L, (starts, lens), words, out=kb[:, :lp].double())
    with pytest.raises(ValueError):
        K.pad_mask_bias(B, L, (starts, lens), words, accumulate=True)
    with pytest.raises(ValueError):
        K.pad_mask_bias(B, L, (starts, lens), words[:2])
    with pytest.raises(ValueError):
        K.pad_mask_rows_fwd(x[:, :L, :D], pe[:5], (starts, lens), words)
    with pytest.raises(ValueError):
        K.pad_mask_rows_bwd(x[:, :L, :D].bfloat16(), (starts, lens), words)
