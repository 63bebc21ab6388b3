"""GPU: direct parity tests of the small kernels of csrc/glue.hip (and the column-sum / dropout
backward pair of csrc/norm.hip) against float64 or exact bit / integer references computed on the
CPU from the same bf16- or fp32-rounded inputs the kernels read.

Every output buffer is larger than the kernel needs and pre-filled with a sentinel (NaN for fp32,
the bit pattern SENT for bf16, a negative constant for int32); the tests assert that the sentinel
survives wherever the kernel must not write (padding columns of strided rows, rows past the end,
gaps between matrices), so an out-of-bounds write fails a test.

Tolerances, each restated in the docstring of the test that uses it:
  * "1 bf16 ulp": |out - ref| <= 2^-8 |ref|. A bf16 has 8 significand bits, so rounding the exact
    value to nearest moves it by at most 2^-9 .. 2^-8 of its magnitude; the fp32 arithmetic in
    front of the rounding is wrong by ~2^-22 relative, which can flip a rounding but stays far
    inside the slack between half an ulp and 2^-8 |ref|.
  * fp32 sums of n terms: n * 2^-24 * sum|terms| (each of at most n roundings is wrong by at most
    2^-24 of a partial sum, itself at most sum|terms|).
  * bit-exact wherever the kernel only moves data, rounds once, or repeats fp32 operations that
    numpy float32 performs with the same correctly rounded result.
No index array handed to a kernel here holds an out-of-range entry (except the embedding ids,
which the gather clamps by construction)."""
import math

import numpy as np
import pytest
import torch

from oracle import rng as R

pytestmark = pytest.mark.gpu

SENT = 0x7FC5            # a bf16 NaN pattern no kernel here produces
U24 = 2.0 ** -24         # fp32 unit roundoff
BF_ULP = 2.0 ** -8       # bf16: relative size of one rounding step (see the module docstring)


def _C():
    from multi_modal_transformers_tokenmerge_amd import _C as C
    return C


def _K():
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    return K


def bf_sentinel(shape, dev):
    return torch.full(shape, SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)


def f32_sentinel(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def bits16(t):
    """bf16 tensor -> its bit patterns as a numpy uint16 array (CPU)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bits32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def f64(t):
    return t.detach().cpu().double().numpy()


def all_sentinel_bf(t):
    return bool((bits16(t) == SENT).all())


def all_nan(t):
    return bool(torch.isnan(t).all().item())


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ sequence assembly
KIND_TEXT, KIND_IMAGE, KIND_READOUT = 0, 1, 2
Q_TAB = 16


class _Seq:
    """One sequence layout: text buffer of T rows (row 1 named by no row_src entry), image buffer
    of NI rows (rows 0 and NI - 2 unnamed), readout table of NR + 1 rows (row 2 unnamed); the L
    named rows interleaved out of order, starting readout, image, text, image."""

    def __init__(self, B, L, D, T, NI, NR, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.L, self.D, self.T, self.NI, self.NR = B, L, D, T, NI, NR
        self.text_used = [j for j in range(T) if j != 1]
        self.img_used = [j for j in range(NI) if j not in (0, NI - 2)]
        self.read_used = [j for j in range(NR + 1) if j != 2]
        ents = ([(KIND_TEXT, j) for j in self.text_used] + [(KIND_IMAGE, j) for j in self.img_used] +
                [(KIND_READOUT, j) for j in self.read_used])
        assert len(ents) == L and len({T, NI, NR}) == 3
        perm = torch.randperm(L, generator=g).tolist()
        ents = [ents[i] for i in perm]
        head = [(KIND_READOUT, self.read_used[-1]), (KIND_IMAGE, self.img_used[-1]),
                (KIND_TEXT, self.text_used[-1]), (KIND_IMAGE, self.img_used[0])]
        self.ents = head + [e for e in ents if e not in head]
        self.row_src = torch.tensor([(k << 24) | j for k, j in self.ents], dtype=torch.int32)
        self.text = torch.randn((B, T, D), generator=g).bfloat16()
        self.img = torch.randn((B, NI, D), generator=g).bfloat16()
        self.rtok = torch.randint(0, Q_TAB, (B, NI), generator=g, dtype=torch.int32)
        self.ctok = torch.randint(0, Q_TAB, (B, NI), generator=g, dtype=torch.int32)
        j0, j1 = self.img_used[0], self.img_used[-1]
        self.rtok[0, j0], self.rtok[B - 1, j1] = 0, Q_TAB - 1      # both ends of the tables
        self.ctok[0, j0], self.ctok[B - 1, j1] = Q_TAB - 1, 0
        self.row_emb = torch.randn((Q_TAB, D), generator=g)
        self.col_emb = torch.randn((Q_TAB, D), generator=g)
        self.readout_pe = torch.randn((NR + 1, D), generator=g)
        self.pe = torch.randn((L, D), generator=g)
        self.dx0 = torch.randn((B, L, D), generator=g)
        self.dro_start = torch.randn((NR + 1, D), generator=g)


SEQ_SHAPES = [  # B, L, D, T, NI, NR: L = (T - 1) + (NI - 2) + NR
    (3, 11, 8, 3, 7, 4),          # one 8-wide chunk per row, 33 threads
    (2, 37, 72, 6, 22, 12),       # 666 threads (no multiple of 256), D / 8 = 9 odd
    (5, 300, 384, 17, 258, 28),   # 72000 threads
]


@pytest.fixture(scope="module", params=SEQ_SHAPES, ids=lambda s: "B%d-L%d-D%d" % s[:3])
def seq(request):
    return _Seq(*request.param, seed=sum(request.param))


def _seq_fwd_refs(s):
    """fp32 restatement in the kernel's association and the float64 value with sum|terms|."""
    B, L, D = s.B, s.L, s.D
    text, img = s.text.float().numpy(), s.img.float().numpy()
    re, ce, rp, pe = (t.numpy() for t in (s.row_emb, s.col_emb, s.readout_pe, s.pe))
    rt, ct = s.rtok.numpy(), s.ctok.numpy()
    r32 = np.empty((B, L, D), np.float32)
    r64 = np.empty((B, L, D), np.float64)
    mag = np.empty((B, L, D), np.float64)
    for l, (kind, j) in enumerate(s.ents):
        if kind == KIND_TEXT:
            terms = [text[:, j]]
            v = text[:, j]
        elif kind == KIND_IMAGE:
            terms = [img[:, j], re[rt[:, j]], ce[ct[:, j]]]
            v = img[:, j] + (re[rt[:, j]] + ce[ct[:, j]])
        else:
            terms = [np.broadcast_to(rp[j], (B, D))]
            v = terms[0]
        terms.append(np.broadcast_to(pe[l], (B, D)))
        r32[:, l] = v + pe[l]
        r64[:, l] = sum(t.astype(np.float64) for t in terms)
        mag[:, l] = sum(np.abs(t.astype(np.float64)) for t in terms)
    assert r32.dtype == np.float32
    return r32, r64, mag


def test_seq_assemble_fwd(dev, seq):
    """mmt_seq_assemble_fwd on interleaved text / image / readout rows. Bit-exact against numpy
    float32 in the kernel's association ((img + (row_emb + col_emb)) + pe), (text + pe),
    (readout_pe + pe): additions only, each correctly rounded on both sides. Against float64 the
    bound is 4 * 2^-24 * sum|terms| (at most 3 roundings of partial sums <= sum|terms|, one
    spare): the bound that still holds if the adds are reordered. The batch row past B keeps its
    NaN sentinel."""
    C, s = _C(), seq
    B, L, D = s.B, s.L, s.D
    d = {k: getattr(s, k).to(dev) for k in ("row_src", "text", "img", "rtok", "ctok", "row_emb",
                                             "col_emb", "readout_pe", "pe")}
    x0 = f32_sentinel((B + 1, L, D), dev)
    C.call("mmt_seq_assemble_fwd", B, L, D, C.ptr(d["row_src"]), C.ptr(d["text"]), s.T,
           C.ptr(d["img"]), s.NI, C.ptr(d["rtok"]), C.ptr(d["ctok"]), C.ptr(d["row_emb"]),
           C.ptr(d["col_emb"]), C.ptr(d["readout_pe"]), C.ptr(d["pe"]), C.ptr(x0), C.stream_ptr())
    sync()
    r32, r64, mag = _seq_fwd_refs(s)
    got = x0[:B].cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), r32.view(np.uint32))
    err = np.abs(got.astype(np.float64) - r64)
    print("seq fwd: max err / bound =", (err / (4 * U24 * mag)).max())
    assert (err <= 4 * U24 * mag).all()
    assert all_nan(x0[B])


def test_seq_assemble_fwd_tokenizer_form(dev):
    """The image tokenizer's own call: image rows only, text = readout_pe = NULL, T = 1, a zero
    position table. Bit-exact with (img + (row_emb + col_emb)) + 0 in numpy float32."""
    C = _C()
    g = torch.Generator().manual_seed(77)
    B, NI, D = 2, 9, 24
    img = torch.randn((B, NI, D), generator=g).bfloat16()
    rt = torch.randint(0, Q_TAB, (B, NI), generator=g, dtype=torch.int32)
    ct = torch.randint(0, Q_TAB, (B, NI), generator=g, dtype=torch.int32)
    rt[0, 0], ct[0, 0], rt[1, NI - 1], ct[1, NI - 1] = 0, Q_TAB - 1, Q_TAB - 1, 0
    re, ce = torch.randn((Q_TAB, D), generator=g), torch.randn((Q_TAB, D), generator=g)
    rows = torch.tensor([(KIND_IMAGE << 24) | j for j in range(NI)], dtype=torch.int32)
    zpe = torch.zeros((NI, D))
    dv = [t.to(dev) for t in (rows, img, rt, ct, re, ce, zpe)]
    out = f32_sentinel((B + 1, NI, D), dev)
    C.call("mmt_seq_assemble_fwd", B, NI, D, C.ptr(dv[0]), None, 1, C.ptr(dv[1]), NI, C.ptr(dv[2]),
           C.ptr(dv[3]), C.ptr(dv[4]), C.ptr(dv[5]), None, C.ptr(dv[6]), C.ptr(out), C.stream_ptr())
    sync()
    ref = (img.float().numpy() + (re.numpy()[rt.numpy()] + ce.numpy()[ct.numpy()])) + np.float32(0)
    np.testing.assert_array_equal(out[:B].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert all_nan(out[B])


def test_seq_assemble_bwd(dev, seq):
    """mmt_seq_assemble_bwd in the training step's form (drow_emb = dcol_emb = NULL). dtext / dimg
    are bit-exact with dx0[...].bfloat16() (one round to nearest even); rows that no row_src entry
    names, and the batch row past B, keep the bf16 sentinel. dreadout_pe is accumulated onto a
    non-zero start by B fp32 atomic adds in unknown order: each add rounds a partial sum that is
    at most |start| + sum_b|dx0| in magnitude, so the bound against the float64 sum is
    B * 2^-24 * (|start| + sum_b|dx0|) per element (the start is a term of the sum like the B
    others); the unnamed table row keeps its start exactly. With dtext = NULL (frozen text encoder)
    dimg and dreadout_pe come out the same."""
    C, s = _C(), seq
    B, L, D, T, NI = s.B, s.L, s.D, s.T, s.NI
    row_src, dx0, rt, ct = (t.to(dev) for t in (s.row_src, s.dx0, s.rtok, s.ctok))

    def run(with_text):
        dtext = bf_sentinel((B + 1, T, D), dev) if with_text else None
        dimg = bf_sentinel((B + 1, NI, D), dev)
        dro = s.dro_start.to(dev).clone()
        C.call("mmt_seq_assemble_bwd", B, L, D, C.ptr(row_src), C.ptr(dx0), C.ptr(dtext), T,
               C.ptr(dimg), NI, C.ptr(rt), C.ptr(ct), None, Q_TAB, None, None, C.ptr(dro),
               C.stream_ptr())
        sync()
        return dtext, dimg, dro

    dtext, dimg, dro = run(True)
    exp_t = np.full((B + 1, T, D), SENT, np.uint16)
    exp_i = np.full((B + 1, NI, D), SENT, np.uint16)
    ref_ro = s.dro_start.double().numpy().copy()
    mag_ro = np.abs(ref_ro)
    for l, (kind, j) in enumerate(s.ents):
        if kind == KIND_TEXT:
            exp_t[:B, j] = bits16(s.dx0[:, l].bfloat16())
        elif kind == KIND_IMAGE:
            exp_i[:B, j] = bits16(s.dx0[:, l].bfloat16())
        else:
            ref_ro[j] += s.dx0[:, l].double().numpy().sum(0)
            mag_ro[j] += s.dx0[:, l].double().abs().numpy().sum(0)
    np.testing.assert_array_equal(bits16(dtext), exp_t)
    np.testing.assert_array_equal(bits16(dimg), exp_i)
    err = np.abs(f64(dro) - ref_ro)
    print("seq bwd dreadout_pe: max err / bound =", (err / (B * U24 * mag_ro)).max())
    assert (err <= B * U24 * mag_ro).all()
    np.testing.assert_array_equal(bits32(dro[2]), bits32(s.dro_start[2]))   # the unnamed row

    none_t, dimg2, dro2 = run(False)
    assert none_t is None
    np.testing.assert_array_equal(bits16(dimg2), exp_i)
    assert (np.abs(f64(dro2) - ref_ro) <= B * U24 * mag_ro).all()


# ----------------------------------------------------------------------------- readout mean
MEAN_B, MEAN_L = 3, 9
MEAN_ROWS = {1: [MEAN_L - 1], 3: [MEAN_L - 1, 0, 7], 4: [MEAN_L - 1, 0, 7, 3]}


def _strided_x(vals, pad_t, pad_b, dev):
    """(B, L, D) fp32 values as a view with row stride D + pad_t and batch stride
    L * (D + pad_t) + pad_b inside a NaN-filled buffer."""
    B, L, D = vals.shape
    xs_t = D + pad_t
    xs_b = L * xs_t + pad_b
    buf = torch.full((B * xs_b,), float("nan"), dtype=torch.float32)
    view = buf.as_strided((B, L, D), (xs_b, xs_t, 1))
    view.copy_(vals)
    return buf.to(dev), xs_b, xs_t


def _rows_mean(dev, vals, rows):
    C = _C()
    B, L, D = vals.shape
    xbuf, xs_b, xs_t = _strided_x(vals, 4, 5, dev)
    assert xs_t > D and xs_b > L * xs_t
    c0, ld_out = 3, D + 7                       # the slot: columns [c0, c0 + D) of a wider row
    out = bf_sentinel((B + 1, ld_out), dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    C.call("mmt_rows_mean_fwd", C.ptr(xbuf), xs_b, xs_t, B, D, C.ptr(rows_d), len(rows),
           out.data_ptr() + 2 * c0, ld_out, C.stream_ptr())
    sync()
    assert all_sentinel_bf(out[:, :c0]) and all_sentinel_bf(out[:, c0 + D:]) and all_sentinel_bf(out[B])
    return out[:B, c0:c0 + D]


@pytest.mark.parametrize("D", [8, 200, 384])
@pytest.mark.parametrize("nrows", [1, 3, 4])
def test_rows_mean_fwd(dev, nrows, D):
    """mmt_rows_mean_fwd on a strided x (xs_t > D, xs_b > L xs_t), unsorted rows [L-1, 0, 7(, 3)],
    a bf16 slot inside a wider row (ld_out > D). Random inputs: within 1 bf16 ulp of the float64
    mean, |out - ref| <= 2^-8 |ref| (the fp32 sum of <= 4 terms and the division are wrong by
    ~2^-22, far below half a bf16 ulp, but may flip one rounding). nrows = 1: bit-exact with
    x.bfloat16(). nrows = 4 with small integers: the mean is a multiple of 1/4 below 8, exact in
    bf16, so bit-exact. Columns outside the slot and the row past B keep the sentinel."""
    g = torch.Generator().manual_seed(100 * nrows + D)
    rows = MEAN_ROWS[nrows]
    vals = torch.randn((MEAN_B, MEAN_L, D), generator=g)
    got = _rows_mean(dev, vals, rows)
    ref = vals[:, rows].double().mean(1).numpy()
    err = np.abs(f64(got) - ref)
    print("rows mean: max err / |ref| =", (err / np.abs(ref)).max(), "bound", BF_ULP)
    assert (err <= BF_ULP * np.abs(ref)).all()
    if nrows == 1:
        np.testing.assert_array_equal(bits16(got), bits16(vals[:, rows[0]].bfloat16()))
    if nrows == 4:
        ints = torch.randint(-8, 9, (MEAN_B, MEAN_L, D), generator=g).float()
        got = _rows_mean(dev, ints, rows)
        exact = ints[:, rows].double().mean(1)
        assert torch.equal(exact.bfloat16().double(), exact)          # representable
        np.testing.assert_array_equal(bits16(got), bits16(exact.bfloat16()))


@pytest.mark.parametrize("D", [8, 200, 384])
@pytest.mark.parametrize("nrows", [1, 3, 4])
def test_rows_mean_bwd(dev, nrows, D):
    """mmt_rows_mean_bwd writes the whole (B, L, D) dx: rows with row_flag >= 0 hold
    fp32(bf16 de) / nrows, within 1 fp32 ulp (2^-23 |ref|) of the float64 quotient (one fp32
    division); every other row is exactly 0.0. de is a slot in a wider row (ld_de > D); the batch
    row past B keeps its NaN sentinel."""
    C = _C()
    g = torch.Generator().manual_seed(200 * nrows + D)
    B, L = MEAN_B, MEAN_L
    rows = MEAN_ROWS[nrows]
    c0, ld_de = 2, D + 5
    de = torch.randn((B, ld_de), generator=g).bfloat16()
    flag = torch.full((L,), -1, dtype=torch.int32)
    for i, r in enumerate(rows):
        flag[r] = i
    de_d, flag_d = de.to(dev), flag.to(dev)
    dx = f32_sentinel((B + 1, L, D), dev)
    C.call("mmt_rows_mean_bwd", de_d.data_ptr() + 2 * c0, ld_de, B, L, D, C.ptr(flag_d), nrows,
           C.ptr(dx), C.stream_ptr())
    sync()
    got = f64(dx[:B])
    ref = np.zeros((B, L, D))
    ref[:, rows] = (de[:, c0:c0 + D].double().numpy() / nrows)[:, None, :]
    on = np.zeros(L, bool)
    on[rows] = True
    assert (np.abs(got[:, on] - ref[:, on]) <= 2.0 ** -23 * np.abs(ref[:, on])).all()
    assert (bits32(dx[:B])[:, ~on] == 0).all()                       # +0.0 exactly
    assert all_nan(dx[B])


# ------------------------------------------------------------------- diffusion noising, loss
STEPS, SEED, STEP = 50, 1234, 7
PREP_B, PREP_BIG = 67, 1067
TIME_W, READ_D = 32, 24            # cat is A + time_dim + D wide


def _prep_inputs(A, F, B, seed):
    g = torch.Generator().manual_seed(seed)
    actions = torch.randn((B, A), generator=g)
    betas = torch.linspace(1e-4, 0.1, STEPS, dtype=torch.float64)
    alpha_hats = torch.cumprod(1 - betas, 0).float()
    fw = (torch.rand((F,), generator=g) * 4 - 2)      # |2 pi t w| up to ~600 rad at t = 49
    if F > 1:
        fw[0], fw[1] = 2.0, -2.0
    else:
        fw[0] = 2.0
    return actions, alpha_hats, fw


def _run_prep(dev, actions, alpha_hats, fw, sample_offset, t_in=None, eps_in=None, drawn=True):
    C = _C()
    B, A = actions.shape
    F = fw.numel()
    ld_cat = A + TIME_W + READ_D
    rng = torch.tensor([SEED, STEP], dtype=torch.int32, device=dev) if drawn else None
    a_d, ah_d, fw_d = actions.to(dev), alpha_hats.to(dev), fw.to(dev)
    t_in_d = None if t_in is None else t_in.to(dev)
    eps_in_d = None if eps_in is None else eps_in.to(dev)
    t_out = torch.full((B + 1,), -7777, dtype=torch.int32, device=dev)
    eps_out = f32_sentinel((B + 1, A), dev)
    cat = bf_sentinel((B + 1, ld_cat), dev)
    feats = bf_sentinel((B + 1, 2 * F), dev)
    C.call("mmt_diffusion_prep", C.ptr(rng), B, A, STEPS, sample_offset, C.ptr(a_d), C.ptr(ah_d),
           C.ptr(fw_d), F, C.ptr(t_in_d), C.ptr(eps_in_d), C.ptr(t_out), C.ptr(eps_out), C.ptr(cat),
           ld_cat, C.ptr(feats), C.stream_ptr())
    sync()
    assert t_out[B].item() == -7777 and all_nan(eps_out[B])
    assert all_sentinel_bf(cat[:, A:]) and all_sentinel_bf(cat[B]) and all_sentinel_bf(feats[B])
    return t_out[:B].cpu(), eps_out[:B].cpu(), cat[:B, :A].cpu(), feats[:B].cpu()


def _check_cat_feats(actions, alpha_hats, fw, t, eps, cat, feats):
    """cat[:, :A] within 1 bf16 ulp (2^-8 |ref|) of float64 sqrt(abar_t) a + sqrt(1 - abar_t) eps
    from the device's own eps; feats within 2^-8 absolute (1 bf16 ulp at 1: outputs lie in
    [-1, 1]) of float64 cos / sin of h, h formed in numpy float32 in the kernel's order
    ((2 pi) t) w: two correctly rounded multiplies, so h is reproducible."""
    ah = alpha_hats.double().numpy()[t.numpy()][:, None]
    ref = np.sqrt(ah) * actions.double().numpy() + np.sqrt(1 - ah) * eps.double().numpy()
    err = np.abs(f64(cat) - ref)
    print("diffusion cat: max err / |ref| =", (err / np.abs(ref)).max(), "bound", BF_ULP)
    assert (err <= BF_ULP * np.abs(ref)).all()
    two_pi = np.float32(2.0) * np.float32(3.141592653589793)
    h = (two_pi * t.numpy().astype(np.float32))[:, None] * fw.numpy()[None, :]
    assert h.dtype == np.float32 and np.abs(h).max() > 300
    ref_f = np.concatenate([np.cos(h.astype(np.float64)), np.sin(h.astype(np.float64))], axis=1)
    err_f = np.abs(f64(feats) - ref_f)
    print("diffusion feats: max abs err =", err_f.max(), "bound", BF_ULP)
    assert (err_f <= BF_ULP).all()


_prep_big_cache = {}


def _prep_big(dev, A, F):
    """One call over PREP_BIG samples at sample_offset 0, shared by the shard checks."""
    if (A, F) not in _prep_big_cache:
        inp = _prep_inputs(A, F, PREP_BIG, 1000 * A + F)
        _prep_big_cache[(A, F)] = (inp, _run_prep(dev, *inp, 0))
    return _prep_big_cache[(A, F)]


@pytest.mark.parametrize("sample_offset", [0, 1000])
@pytest.mark.parametrize("A,F", [(8, 96), (7, 300), (7, 1), (8, 300)])
def test_diffusion_prep_drawn(dev, A, F, sample_offset):
    """mmt_diffusion_prep drawing t and eps on the device (t_in = eps_in = NULL), B = 67.
    t: bit-exact with oracle.rng.diffusion_t_eps, in [0, steps). Shard property: the call at
    sample_offset s equals rows [s, s + 67) of one 1067-sample call bit for bit (t, eps, cat,
    feats). eps against a float64 Box-Muller of the same integer draws (u1, u2 formed as the
    oracle forms them, log / sqrt / cos in float64), absolute tolerance 1e-5:
    |sqrt(-2 ln u1)| <= sqrt(48 ln 2) ~ 5.8; the fp32 argument 2 pi u2 <= 6.29 carries at most
    4.8e-7 of rounding, cosf adds ~1e-7; together ~4e-6. cat / feats: see _check_cat_feats.
    Columns [A, ld_cat) of cat and every row past B keep their sentinels."""
    (act_big, ah, fw), (t_big, eps_big, cat_big, feats_big) = _prep_big(dev, A, F)
    sl = slice(sample_offset, sample_offset + PREP_B)
    actions = act_big[sl].contiguous()
    t, eps, cat, feats = _run_prep(dev, actions, ah, fw, sample_offset)
    t_ref, _ = R.diffusion_t_eps(SEED, STEP, PREP_B, A, STEPS, sample_offset)
    np.testing.assert_array_equal(t.numpy(), t_ref)
    assert ((t.numpy() >= 0) & (t.numpy() < STEPS)).all()
    np.testing.assert_array_equal(t.numpy(), t_big[sl].numpy())
    np.testing.assert_array_equal(bits32(eps), bits32(eps_big[sl]))
    np.testing.assert_array_equal(bits16(cat), bits16(cat_big[sl]))
    np.testing.assert_array_equal(bits16(feats), bits16(feats_big[sl]))
    b = np.arange(PREP_B, dtype=np.uint64) + np.uint64(sample_offset)
    ke = R.stream_key(SEED, STEP, 0xFFFE, 2)
    c = (b[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]) & R.M32
    d1 = R.draw_u32(ke, (np.uint64(2) * c) & R.M32)
    d2 = R.draw_u32(ke, (np.uint64(2) * c + np.uint64(1)) & R.M32)
    u1 = ((d1 >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    u2 = (d2 >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    eps_ref = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))
    err = np.abs(f64(eps) - eps_ref)
    print("diffusion eps: max abs err =", err.max(), "bound 1e-5")
    assert (err <= 1e-5).all()
    _check_cat_feats(actions, ah, fw, t, eps, cat, feats)


@pytest.mark.parametrize("A,F", [(8, 96), (7, 300), (8, 1)])
def test_diffusion_prep_injected(dev, A, F):
    """mmt_diffusion_prep with t_in / eps_in given (rng NULL): t_out and eps_out are bit copies,
    t covers 0 and steps - 1; cat / feats as on the drawn path (see _check_cat_feats)."""
    B = 13
    actions, ah, fw = _prep_inputs(A, F, B, 31 * A + F)
    g = torch.Generator().manual_seed(A + F)
    t_in = torch.randint(0, STEPS, (B,), generator=g, dtype=torch.int32)
    t_in[0], t_in[B - 1], t_in[5] = 0, STEPS - 1, STEPS - 1
    eps_in = torch.randn((B, A), generator=g)
    t, eps, cat, feats = _run_prep(dev, actions, ah, fw, 0, t_in=t_in, eps_in=eps_in, drawn=False)
    np.testing.assert_array_equal(t.numpy(), t_in.numpy())
    np.testing.assert_array_equal(bits32(eps), bits32(eps_in))
    _check_cat_feats(actions, ah, fw, t, eps, cat, feats)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("B,A", [(1, 5), (128, 8), (205, 5), (513, 8)])
def test_diffusion_loss(dev, B, A, grad_scale):
    """mmt_diffusion_loss at B A = 5 (below one wave), 1024 (one pass of the 1024 threads), 1025
    and 4104 (several passes), ld_pred > A. loss against float64 mean_b sum_j 0.5 (pred - eps)^2
    at rtol 1e-5: all terms are positive and the longest chain is ceil(B A / 1024) + 6 + 16 fp32
    roundings, <= 27 * 2^-24 = 1.6e-6 relative, plus 3 roundings per term. loss is overwritten
    (it starts at a sentinel), the word after it keeps its own. dpred within 1 bf16 ulp
    (2^-8 |ref|) of float64 (pred - eps) grad_scale / B: the fp32 difference is correctly
    rounded, so no cancellation is hidden. The elements past B A keep the bf16 sentinel."""
    C = _C()
    g = torch.Generator().manual_seed(B * A)
    ld_pred = A + 3
    pred = torch.randn((B, ld_pred), generator=g)
    eps = torch.randn((B, A), generator=g)
    pred_d, eps_d = pred.to(dev), eps.to(dev)
    loss = torch.tensor([12345.0, float("nan")], device=dev)
    dpred = bf_sentinel((B * A + 9,), dev)
    C.call("mmt_diffusion_loss", C.ptr(pred_d), ld_pred, C.ptr(eps_d), B, A, grad_scale,
           C.ptr(loss), C.ptr(dpred), C.stream_ptr())
    sync()
    d = pred[:, :A].double().numpy() - eps.double().numpy()
    ref_loss = (0.5 * d * d).sum() / B
    got_loss = float(loss[0].item())
    print("diffusion loss:", got_loss, "ref", ref_loss, "rel", abs(got_loss - ref_loss) / ref_loss)
    assert abs(got_loss - ref_loss) <= 1e-5 * ref_loss
    assert math.isnan(loss[1].item())
    ref_d = d * grad_scale / B
    err = np.abs(f64(dpred[:B * A]).reshape(B, A) - ref_d)
    assert (err <= BF_ULP * np.abs(ref_d)).all()
    assert all_sentinel_bf(dpred[B * A:])


# -------------------------------------------------------------------------- batched transpose
def _transpose_case(dev, shapes, src_gap, dst_gap):
    """Descriptor as ParamStore builds it ({src_off, dst_off, rows, cols, first_tile}, first_tile
    the running count of 64 x 64 tiles), matrices at non-adjacent offsets with src_off != dst_off;
    returns (got dst bits, expected dst bits) over the whole dst buffer."""
    C = _C()
    desc, tiles, so, do = [], 0, 3, 10
    for r, c in shapes:
        desc += [so, do, r, c, tiles]
        tiles += -(-r // 64) * -(-c // 64)
        so += r * c + src_gap
        do += r * c + dst_gap
    src = (np.arange(so, dtype=np.int64) % 65521).astype(np.uint16)     # a counter as bf16 bits
    exp = np.full(do, 0xFFFF, np.uint16)                                # sentinel in every gap
    for i, (r, c) in enumerate(shapes):
        s0, d0 = desc[5 * i], desc[5 * i + 1]
        exp[d0:d0 + r * c] = src[s0:s0 + r * c].reshape(r, c).T.reshape(-1)
    src_d = torch.from_numpy(src.view(np.int16)).to(dev).view(torch.bfloat16)
    dst_d = torch.from_numpy(np.full(do, 0xFFFF, np.uint16).view(np.int16)).to(dev).view(torch.bfloat16)
    desc_d = torch.tensor(desc, dtype=torch.int64, device=dev)
    C.call("mmt_transpose_bf16_batched", C.ptr(src_d), C.ptr(dst_d), C.ptr(desc_d), len(shapes),
           tiles, C.stream_ptr())
    sync()
    return bits16(dst_d), exp, tiles


def test_transpose_batched_mixed_shapes(dev):
    """mmt_transpose_bf16_batched over (64, 64), (65, 130), (8, 384), (1, 7), (200, 3) in one call:
    full tiles, partial last tiles in both directions, single rows and thin matrices. Bit-exact
    over the whole dst buffer, gaps (sentinel 0xFFFF) included; distinct source values show any
    misplaced element."""
    got, exp, tiles = _transpose_case(dev, [(64, 64), (65, 130), (8, 384), (1, 7), (200, 3)], 5, 11)
    assert tiles == 1 + 6 + 6 + 1 + 4
    np.testing.assert_array_equal(got, exp)


def test_transpose_batched_many_matrices(dev):
    """5000 matrices of (3, 5): 5000 tiles, past the launch's 4096 workgroups, so the grid-stride
    loop and the descriptor scan both run beyond the first pass. Bit-exact, gaps included."""
    got, exp, tiles = _transpose_case(dev, [(3, 5)] * 5000, 1, 2)
    assert tiles == 5000 > 4096
    np.testing.assert_array_equal(got, exp)


def test_transpose_batched_one_large_matrix(dev):
    """A single (64 * 65, 64 * 64) matrix: 4160 tiles (past the 4096 workgroups) of one
    descriptor, 34 MB. Bit-exact, the elements after its end keep the sentinel."""
    got, exp, tiles = _transpose_case(dev, [(64 * 65, 64 * 64)], 0, 7)
    assert tiles == 4160
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------------------- T5 pieces
RMS_EPS = 1e-6


@pytest.mark.parametrize("rows", [1, 5, 4099])
@pytest.mark.parametrize("D", [8, 64, 504, 512, 520, 1024, 1032, 2048])
def test_rmsnorm(dev, D, rows):
    """mmt_rmsnorm_fwd (four rows per workgroup; D <= 1024: each lane reads its two chunks once,
    lanes past D idle; D > 1024: the loop). Against float64 x rsqrt(mean(x^2) + eps) w on the bf16
    inputs: |y - ref| <= 2^-8 |ref| + 2^-133, 1 bf16 ulp (the fp32 sum, rsqrtf and two multiplies
    are wrong by ~2^-22) plus bf16's smallest subnormal. A row of zeros gives zeros, not NaN
    (eps > 0). A row holding one element of 3e38 magnitude: the kernel's fp32 sum of squares
    overflows to inf, rsqrtf(inf) = 0 and the whole output row is zero, where the float64
    reference gives +-sqrt(D) w for that element and ~0 for the rest; that row is asserted to be
    zero and left out of the comparison (a documented limit of the fp32 accumulation, no T5
    activation comes near it). The rows past `rows` keep the sentinel."""
    K = _K()
    g = torch.Generator().manual_seed(D + rows)
    x = (torch.randn((rows, D), generator=g) * 3).bfloat16()
    w = (torch.randn((D,), generator=g) + 1).bfloat16()
    w[D // 2] = 1.5
    zero_row = huge_row = None
    if rows >= 5:
        zero_row, huge_row = 2, 3
        x[zero_row] = 0
        x[huge_row, D // 2] = 3e38
    y = bf_sentinel((rows + 2, D), dev)
    K.rmsnorm(x.to(dev), w.to(dev), RMS_EPS, out=y)
    sync()
    assert all_sentinel_bf(y[rows:])
    got = f64(y[:rows])
    x64, w64 = x.double().numpy(), w.double().numpy()
    ref = x64 / np.sqrt((x64 * x64).mean(1, keepdims=True) + RMS_EPS) * w64
    cmp = np.ones(rows, bool)
    if huge_row is not None:
        cmp[huge_row] = False
        assert (got[huge_row] == 0).all() and np.abs(ref[huge_row]).max() > 1
        assert (got[zero_row] == 0).all()
    err = np.abs(got - ref)[cmp]
    bound = (BF_ULP * np.abs(ref) + 2.0 ** -133)[cmp]
    print("rmsnorm: max err / bound =", (err / bound).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("D,n", [(8, 13), (512, 5), (768, 7)])
def test_embedding_gather(dev, D, n):
    """mmt_embedding_gather, bit-exact with table[ids]; n D / 8 (13, 320, 672 threads) is no
    multiple of 256. ids cover 0 and vocab - 1; -1 and vocab clamp to rows 0 and vocab - 1 (the
    kernel clamps before it forms any address). The row past n keeps the sentinel."""
    K = _K()
    g = torch.Generator().manual_seed(D)
    vocab = 11
    table = torch.randint(-32768, 32768, (vocab, D), generator=g, dtype=torch.int32).to(torch.int16)
    ids = torch.randint(0, vocab, (n,), generator=g, dtype=torch.int32)
    ids[0], ids[1], ids[2], ids[3] = -1, vocab, vocab - 1, 0
    out = bf_sentinel((n + 1, D), dev)
    K.embedding_gather(ids.to(dev), table.to(dev).view(torch.bfloat16), out=out)
    sync()
    exp = table.numpy().view(np.uint16)[np.clip(ids.numpy(), 0, vocab - 1)]
    np.testing.assert_array_equal(bits16(out[:n]), exp)
    assert all_sentinel_bf(out[n])


# ------------------------------------------------------------------- casts and reductions
CAST_SPECIALS = [
    0x3F818000,              # tie, odd below: rounds up to even (0x3F82)
    0x3F808000,              # tie, even below: rounds down to even (0x3F80)
    0x7F7FFFFF,              # largest finite fp32: rounds to +inf
    0x00000000, 0x80000000,  # +-0
    0x7F800000, 0xFF800000,  # +-inf
    0x7FC00000,              # NaN (index CAST_NAN)
    0x00000001, 0x807FFFFF, 0x00400000, 0x00008000, 0x00018000,   # fp32 subnormals
    0xFF7FFFFF, 0x3F808001, 0x3F817FFF, 0xBF818000,
]
CAST_NAN = 7


@pytest.mark.parametrize("n", [1, 255, 257, 2 ** 19 + 3])
def test_cast_f32_bf16(dev, n):
    """mmt_cast_f32_bf16 is bit-exact with torch.Tensor.bfloat16() (round to nearest even) on
    +-0, +-inf, fp32 subnormals, the largest finite fp32 (-> inf), both tie patterns and random
    values; the NaN stays a NaN. n = 2^19 + 3 exceeds the 2048 x 256 threads of the capped launch
    (grid-stride loop). The element after the end keeps the sentinel."""
    K = _K()
    g = torch.Generator().manual_seed(n)
    a = torch.randn((n,), generator=g) * 100
    k = min(n, len(CAST_SPECIALS))
    a[:k] = torch.from_numpy(np.array(CAST_SPECIALS[:k], np.uint32).view(np.float32))
    out = bf_sentinel((n + 1,), dev)
    K.cast_f32_bf16(a.to(dev), out[:n])
    sync()
    got, exp = bits16(out[:n]), bits16(a.bfloat16())
    if n > CAST_NAN:
        assert (got[CAST_NAN] & 0x7F80) == 0x7F80 and (got[CAST_NAN] & 0x7F) != 0   # still a NaN
        got[CAST_NAN] = exp[CAST_NAN]
    np.testing.assert_array_equal(got, exp)
    assert all_sentinel_bf(out[n:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [1, 31, 1000])
@pytest.mark.parametrize("N", [8, 72, 384])
def test_colsum(dev, N, M, dtype):
    """mmt_colsum on a strided x (ldx = N + 8 > N) accumulating onto a non-zero out; N = 72 leaves
    the last 64-column workgroup partial. Against float64: M * 2^-24 * sum_m|x| (fp32 partial
    sums of M terms) plus the accumulator's own ulp, 2^-23 |result| (the atomic adds onto out).
    The words after out keep their NaN sentinel."""
    K = _K()
    g = torch.Generator().manual_seed(M * N)
    ldx = N + 8
    xb = torch.randn((M, ldx), generator=g).to(dtype)
    start = torch.randn((N,), generator=g)
    acc = f32_sentinel((N + 8,), dev)
    acc[:N] = start.to(dev)
    K.colsum(xb.to(dev)[:, :N], acc[:N])
    sync()
    x64 = xb[:, :N].double().numpy()
    ref = start.double().numpy() + x64.sum(0)
    bound = M * U24 * np.abs(x64).sum(0) + 2.0 ** -23 * np.abs(ref)
    err = np.abs(f64(acc[:N]) - ref)
    print("colsum: max err / bound =", (err / bound).max())
    assert (err <= bound).all()
    assert all_nan(acc[N:])


def test_dropout_bwd_cast_and_wrapped_counter(dev):
    """mmt_dropout_bwd on fp32 dy with ldy > N and ldz > N. rng = NULL, colsum = NULL: a pure
    cast, bit-exact with dy.bfloat16(). With rng and a row_offset for which (row_offset + m) N
    crosses 2^32 inside the M rows: the keep mask equals oracle.rng.dropout_mask_2d (which wraps
    the counter to 32 bits) element for element, kept values are within 1 bf16 ulp (2^-8 |ref|)
    of float64 dy / keep_prob (the fp32 1 / 0.9f differs from 1 / 0.9 by 3e-8), dropped ones are
    zero, and colsum (non-zero start) is within M * 2^-24 * sum_m|z| + 2^-23 |result| of the
    float64 column sums. Padding columns and the row past M keep the sentinel."""
    K = _K()
    g = torch.Generator().manual_seed(9)
    M, N = 31, 72
    ldy, ldz = N + 8, N + 16
    dy = torch.randn((M, ldy), generator=g)
    dy_d = dy.to(dev)

    z = bf_sentinel((M + 1, ldz), dev)
    K.dropout_bwd(dy_d[:, :N], None, 0, 0, 1.0, out=z[:M, :N])
    sync()
    np.testing.assert_array_equal(bits16(z[:M, :N]), bits16(dy[:, :N].bfloat16()))
    assert all_sentinel_bf(z[:, N:]) and all_sentinel_bf(z[M])

    kp, layer, site = 0.9, 3, 1
    row_offset = 2 ** 32 // N - 15
    assert row_offset * N < 2 ** 32 < (row_offset + M - 1) * N
    rng = torch.tensor([SEED, STEP], dtype=torch.int32, device=dev)
    start = torch.randn((N,), generator=g)
    cs = f32_sentinel((N + 8,), dev)
    cs[:N] = start.to(dev)
    z = bf_sentinel((M + 1, ldz), dev)
    K.dropout_bwd(dy_d[:, :N], rng, layer, site, kp, row_offset=row_offset, out=z[:M, :N],
                  colsum_out=cs[:N])
    sync()
    keep = R.dropout_mask_2d(SEED, STEP, layer, site, M, N, row_offset, kp)
    assert 0.8 < keep.mean() < 0.97
    got = f64(z[:M, :N])
    np.testing.assert_array_equal(got != 0, keep)                  # dy has no zeros
    ref = np.where(keep, dy[:, :N].double().numpy() / kp, 0.0)
    assert (np.abs(got - ref) <= BF_ULP * np.abs(ref)).all()
    assert all_sentinel_bf(z[:, N:]) and all_sentinel_bf(z[M])
    ref_cs = start.double().numpy() + ref.sum(0)
    bound = M * U24 * np.abs(ref).sum(0) + 2.0 ** -23 * np.abs(ref_cs)
    # the kernel sums dy * fp32(1 / 0.9f): 2^-24-level relative offset of every term from ref
    bound += 2 * U24 * np.abs(ref).sum(0)
    assert (np.abs(f64(cs[:N]) - ref_cs) <= bound).all()
    assert all_nan(cs[N:])
