"""The grouped optimizer launches on the GPU (include/mmt_api.h mmt_adamw_groups /
mmt_optim_prepare_groups), through the raw C ABI, at sizes around the partition edges:

1. no bit set: bit-equal to mmt_adamw / mmt_adamw_dev;
2. random per-chunk flags: decayed chunks bit-equal to the plain kernel, undecayed ones to the
   plain kernel with wd = 0, frozen ones byte-identical to what they held, NaN / Inf gradients
   there notwithstanding;
3. prepare: bit-equal to mmt_optim_prepare with no frozen bit; the trainable norm vs float64 to the
   header's chain bound, reproducible, blind to frozen NaN / Inf; all frozen: norm 0, clip 1;
4. the skip word leaves everything untouched;
5. one captured graph of prepare + AdamW + step advance over a moving schedule equals the eager steps;
6. argument errors are reported, not faults.
"""
import ctypes

import numpy as np
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd.schedules import Constant, WarmupCosine

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit round-off
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 1e-2
NO_DECAY, FROZEN = 1, 2


def _C():
    from multi_modal_transformers_tokenmerge_amd import _C as C
    return C


def _sizes():
    G = _C().GRAD_NORM_GRID
    return [1, 63, 64, 65, 255, G * 1024 - 1, G * 1024, G * 1024 + 1, 1_000_003]


def _chain(n: int) -> int:
    """include/mmt_api.h: ceil(per / 1024) + 13 roundings on the longest path to sum g^2."""
    per = -(-(n // 4) // _C().GRAD_NORM_GRID)
    return -(-per // 1024) + 13


def _bufs(dev, n, seed):
    """(p, m, v, shadow) with non-trivial contents, and a gradient."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    p = torch.randn(n, generator=gen, device=dev)
    m = torch.randn(n, generator=gen, device=dev) * 0.1
    v = torch.rand(n, generator=gen, device=dev) * 0.01
    g = torch.randn(n, generator=gen, device=dev)
    return [p, m, v, p.to(torch.bfloat16)], g


def _clone(bufs):
    return [t.clone() for t in bufs]


def _state(dev, step=0):
    return torch.tensor([1234, step], dtype=torch.int32, device=dev)


def _opt_words(dev, lr, gmul, skip=0.0):
    return torch.tensor([0, 1, gmul, lr, 0, 0, skip, 0], dtype=torch.float32, device=dev)


def _plain(bufs, g, state, lr, wd, gs, opt=None):
    C = _C()
    p, m, v, sh = bufs
    if opt is None:
        C.call("mmt_adamw", C.ptr(p), C.ptr(g), C.ptr(m), C.ptr(v), C.ptr(sh), p.numel(),
               C.ptr(state), lr, B1, B2, EPS, wd, gs, C.stream_ptr())
    else:
        C.call("mmt_adamw_dev", C.ptr(p), C.ptr(g), C.ptr(m), C.ptr(v), C.ptr(sh), p.numel(),
               C.ptr(state), C.ptr(opt), B1, B2, EPS, wd, C.stream_ptr())


def _grouped(bufs, g, state, flags, lr, wd, gs, opt=None, chunk=64):
    C = _C()
    p, m, v, sh = bufs
    assert flags is None or flags.numel() == -(-p.numel() // 64)  # the kernel indexes i >> 6
    C.call("mmt_adamw_groups", C.ptr(p), C.ptr(g), C.ptr(m), C.ptr(v), C.ptr(sh), p.numel(),
           C.ptr(state), C.ptr(opt), lr, B1, B2, EPS, wd, gs, C.ptr(flags), chunk, C.stream_ptr())


def _flags(n, dev, base=0, seed=None, values=(0, 1, 2, 3)):
    """One byte per 64 elements. seed None: values cycled from `base` (chunk 0 takes
    values[base]); else a seeded permutation of that cycle: every value present once there are
    len(values) chunks."""
    nc = -(-n // 64)
    f = torch.tensor(values, dtype=torch.uint8)[(torch.arange(nc) + base) % len(values)]
    if seed is not None:
        f = f[torch.randperm(nc, generator=torch.Generator().manual_seed(seed))]
    return f.to(dev)


def _per_element(flags, n):
    return flags.repeat_interleave(64)[:n]


def _poison(g, frozen_mask):
    """NaN and Inf, alternating, wherever the mask is set."""
    bad = torch.where(torch.arange(g.numel(), device=g.device) % 2 == 0, float("nan"), float("inf"))
    return torch.where(frozen_mask, bad.to(g.dtype), g)


def _same(a, b):
    """Bitwise equality (NaN payloads included)."""
    ia = a.view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.view(torch.int16 if b.element_size() == 2 else torch.int32)
    return torch.equal(ia, ib)


NAMES = ("p", "m", "v", "shadow")


@pytest.mark.parametrize("dev_form", [False, True], ids=["host", "opt"])
def test_no_bit_set_equals_the_plain_kernels(dev, dev_form):
    lr, gs = 3e-3, 0.5
    for n in _sizes():
        a, g = _bufs(dev, n, 11)
        b = _clone(a)
        state = _state(dev, 3)
        opt = _opt_words(dev, lr, gs) if dev_form else None
        flags = torch.zeros(-(-n // 64), dtype=torch.uint8, device=dev)
        for _ in range(2):
            _grouped(a, g, state, flags, lr, WD, gs, opt)
            _plain(b, g, state, lr, WD, gs, opt)
        torch.cuda.synchronize()
        for x, y, name in zip(a, b, NAMES):
            assert _same(x, y), (n, name)
        assert not _same(a[0], _bufs(dev, n, 11)[0][0])  # the step moved the parameters


@pytest.mark.parametrize("dev_form", [False, True], ids=["host", "opt"])
def test_random_flags(dev, dev_form):
    lr, gs = 3e-3, 0.5
    for n in _sizes():
        nc = -(-n // 64)
        # fewer chunks than flag values: every value in turn; else one seeded table with all four
        tables = ([_flags(n, dev, base) for base in range(4)] if nc < 4
                  else [_flags(n, dev, seed=n)])
        seen = set()
        for flags in tables:
            seen |= set(flags.tolist())
            ef = _per_element(flags, n)
            frozen, undecayed = (ef & FROZEN) != 0, (ef & NO_DECAY) != 0
            start, g = _bufs(dev, n, 12)
            g_bad = _poison(g, frozen)
            state = _state(dev, 5)
            opt = _opt_words(dev, lr, gs) if dev_form else None
            got, with_wd, no_wd = _clone(start), _clone(start), _clone(start)
            _grouped(got, g_bad, state, flags, lr, WD, gs, opt)
            _plain(with_wd, g, state, lr, WD, gs, opt)
            _plain(no_wd, g, state, lr, 0.0, gs, opt)
            torch.cuda.synchronize()
            for x, s0, a, b, name in zip(got, start, with_wd, no_wd, NAMES):
                want = torch.where(frozen, s0, torch.where(undecayed, b, a))
                assert _same(x, want), (n, name, flags[:8].tolist())
                if bool(frozen.any()):
                    assert _same(x[frozen], s0[frozen]), (n, name)
            if bool((~frozen).any()):
                assert bool(torch.isfinite(got[0][~frozen]).all())
            sel = ~frozen & ~undecayed
            if bool(sel.any()):
                assert not _same(with_wd[0][sel], no_wd[0][sel])  # wd does show in the bits
        assert seen == {0, 1, 2, 3}, n


def _prep_bufs(dev):
    C = _C()
    opt = torch.zeros(C.OPT_WORDS, dtype=torch.float32, device=dev)
    ws = torch.full((C.workspace_size(C.WS_GRAD_NORM, 1) // 4,), float("nan"), device=dev)
    return opt, ws


def _prepare(g, opt, ws, state, flags=None, grad_scale=1.0, max_norm=0.0, skip=0, sched=None,
             chunk=64):
    C = _C()
    sc = (sched or Constant(1e-3)).to_c()
    head = (C.ptr(g), g.numel(), grad_scale, max_norm, skip, ctypes.addressof(sc), C.ptr(state),
            C.ptr(opt), C.ptr(ws), ws.numel() * 4)
    if flags is None:
        C.call("mmt_optim_prepare", *head, C.stream_ptr())
    else:
        assert flags.numel() == -(-g.numel() // 64)
        C.call("mmt_optim_prepare_groups", *head, C.ptr(flags), chunk, C.stream_ptr())


def test_prepare_without_frozen_bit_equals_plain(dev):
    sched = WarmupCosine(1e-4, 3e-3, 2, 6, 1e-4)
    for n in _sizes():
        _, g = _bufs(dev, n, 13)
        state = _state(dev, 1)
        flags = _flags(n, dev, seed=n, values=(0, NO_DECAY))
        o1, ws1 = _prep_bufs(dev)
        o2, ws2 = _prep_bufs(dev)
        _prepare(g, o1, ws1, state, None, 0.5, 0.25, 1, sched)
        _prepare(g, o2, ws2, state, flags, 0.5, 0.25, 1, sched)
        torch.cuda.synchronize()
        assert _same(o1, o2), (n, o1.tolist(), o2.tolist())
        assert _same(ws1, ws2), n  # every partial, too
        if n >= 255:
            assert float(o1[1]) < 1.0  # the clip is active: gmul carries it


def test_prepare_sees_the_trainable_gradient_only(dev):
    for n in _sizes():
        _, g = _bufs(dev, n, 14)
        flags = _flags(n, dev, seed=n + 1) if n > 255 else _flags(n, dev)  # chunk 0 trainable
        frozen = (_per_element(flags, n) & FROZEN) != 0
        g_bad = _poison(g, frozen)
        ref = float(g.double()[~frozen].norm())
        state = _state(dev)
        got = []
        for _ in range(2):
            opt, ws = _prep_bufs(dev)  # workspace full of NaN: every partial must be written
            _prepare(g_bad, opt, ws, state, flags, skip=1)
            got.append((opt.cpu(), ws.cpu()))
        (o, w), (o2, w2) = got
        A = _chain(n)
        rel = abs(float(o[0]) - ref) / ref
        print(f"n={n}: frozen {int(frozen.sum())} A={A} norm={float(o[0])!r} float64={ref!r} "
              f"rel={rel:.3e} bound={(A + 1) * U:.3e}")
        assert bool(torch.isfinite(w).all()), n
        assert rel <= (A + 1) * U, (n, rel)
        assert _same(o, o2) and _same(w, w2), n
        assert o[1:].tolist() == [1.0, 1.0, np.float32(1e-3), 0.0, 0.0, 0.0, 0.0], (n, o.tolist())
        if n > 255:
            assert bool(frozen.any()) and bool((~frozen).any())


def test_prepare_all_frozen(dev):
    for n in (1, 65, 1_000_003):
        g = torch.full((n,), float("nan"), device=dev)
        flags = torch.full((-(-n // 64),), FROZEN, dtype=torch.uint8, device=dev)
        flags[::2] |= NO_DECAY
        opt, ws = _prep_bufs(dev)
        _prepare(g, opt, ws, _state(dev), flags, grad_scale=0.5, max_norm=1.0, skip=1)
        o = opt.cpu()
        assert o.tolist() == [0.0, 1.0, 0.5, np.float32(1e-3), 0.0, 0.0, 0.0, 0.0], (n, o.tolist())
        assert bool((ws == 0).all()), n


def test_skip_word_leaves_everything_untouched(dev):
    n = 100_003
    start, g = _bufs(dev, n, 15)
    got = _clone(start)
    flags = _flags(n, dev, seed=3)
    _grouped(got, g, _state(dev), flags, 0.0, WD, 0.0, _opt_words(dev, 3e-3, 1.0, skip=1.0))
    torch.cuda.synchronize()
    for x, s0, name in zip(got, start, NAMES):
        assert _same(x, s0), name


def test_one_graph_over_a_moving_schedule(dev):
    C = _C()
    n, steps = 100_003, 5
    sched = WarmupCosine(0.0, 3e-3, 2, 6, 1e-4)
    flags = _flags(n, dev, seed=4)
    frozen = (_per_element(flags, n) & FROZEN) != 0
    start, _ = _bufs(dev, n, 16)
    gen = torch.Generator(device=dev).manual_seed(17)
    grads = [_poison(torch.randn(n, generator=gen, device=dev) * (i + 1), frozen)
             for i in range(steps)]
    g = torch.empty(n, device=dev)

    def one_step(bufs, state, opt, ws):
        _prepare(g, opt, ws, state, flags, 0.5, 1.0, 1, sched)
        _grouped(bufs, g, state, flags, 0.0, WD, 0.0, opt)
        C.call("mmt_step_advance", C.ptr(state), C.stream_ptr())

    eager, state = _clone(start), _state(dev)
    opt, ws = _prep_bufs(dev)
    lrs = []
    for i in range(steps):
        g.copy_(grads[i])
        one_step(eager, state, opt, ws)
        lrs.append(float(opt[3]))
        assert float(opt[1]) < 1.0 and float(opt[6]) == 0.0
    assert len(set(lrs)) >= 4 and int(state[1]) == steps

    graphed, state2 = _clone(start), _state(dev)
    opt2, ws2 = _prep_bufs(dev)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        one_step(graphed, state2, opt2, ws2)
    for t, s0 in zip(graphed + [state2], start + [_state(dev)]):  # capture ran nothing: be sure
        t.copy_(s0)
    opt2.zero_()
    lrs2 = []
    for i in range(steps):
        g.copy_(grads[i])
        graph.replay()
        lrs2.append(float(opt2[3]))
    torch.cuda.synchronize()
    assert lrs2 == lrs and int(state2[1]) == steps
    for x, y, s0, name in zip(graphed, eager, start, NAMES):
        assert _same(x, y), name
        assert _same(x[frozen], s0[frozen]), name
    assert not _same(graphed[0], start[0])


def test_argument_errors(dev):
    C = _C()
    n = 1000
    bufs, g = _bufs(dev, n, 18)
    flags = _flags(n, dev)
    state = _state(dev)
    before = _clone(bufs)
    with pytest.raises(C.MMTError, match="mmt_adamw_groups: null chunk_flags"):
        _grouped(bufs, g, state, None, 1e-3, WD, 1.0)
    for chunk in (0, 32, 128):
        with pytest.raises(C.MMTError, match=f"mmt_adamw_groups: chunk {chunk} != 64"):
            _grouped(bufs, g, state, flags, 1e-3, WD, 1.0, chunk=chunk)
    p, m, v, sh = bufs
    rc = C.lib().mmt_adamw_groups(C.ptr(p), C.ptr(g), C.ptr(m), C.ptr(v), C.ptr(sh), n,
                                  C.ptr(state), None, 1e-3, B1, B2, EPS, WD, 1.0, None, 64,
                                  C.stream_ptr())
    assert rc == -1 and b"chunk_flags" in C.lib().mmt_last_error()  # MMT_ERR_INVALID

    opt, ws = _prep_bufs(dev)
    with pytest.raises(C.MMTError, match="mmt_optim_prepare_groups: null chunk_flags"):
        sc = Constant(1e-3).to_c()
        C.call("mmt_optim_prepare_groups", C.ptr(g), n, 1.0, 0.0, 0, ctypes.addressof(sc),
               C.ptr(state), C.ptr(opt), C.ptr(ws), ws.numel() * 4, None, 64, C.stream_ptr())
    with pytest.raises(C.MMTError, match="mmt_optim_prepare_groups: chunk 16 != 64"):
        _prepare(g, opt, ws, state, flags, chunk=16)
    with pytest.raises(C.MMTError, match="mmt_optim_prepare_groups: g must be 16-B aligned"):
        sc = Constant(1e-3).to_c()
        C.call("mmt_optim_prepare_groups", C.ptr(g[1:]), n - 1, 1.0, 0.0, 0, ctypes.addressof(sc),
               C.ptr(state), C.ptr(opt), C.ptr(ws), ws.numel() * 4, C.ptr(flags), 64,
               C.stream_ptr())
    torch.cuda.synchronize()
    for x, y in zip(bufs, before):  # nothing was launched
        assert _same(x, y)
    assert bool((opt == 0).all())
