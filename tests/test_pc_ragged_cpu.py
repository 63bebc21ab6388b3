"""CPU: the restatement of the ragged point clouds and of the depth back-projection's selection
rule (tests/pc_ragged_ref.py) against answers derived by hand, and the Python surface's argument
plumbing that needs no device."""
import inspect

import numpy as np
import pytest

from tests import pc_ragged_ref as G
from tests import pointcloud_ref as R


def _line(c, n=4, k=3, start=None):
    pts = R.line_cloud()[None, None]
    st = None if start is None else np.array([[start]], np.int32)
    ci, ni, fault = G.sample_group_counts(pts, n, k, np.array([[c]], np.int32), st)
    return ci[0, 0].tolist(), ni[0, 0].tolist(), fault


def test_line_cloud_with_a_count():
    """x = 0 .. 7 on a line, the first c points valid; n = 4 centroids, k = 3 neighbours."""
    # c = 5: 0, the farthest 4, the middle 2, then 1 and 3 tie at d = 1: the lower index
    assert _line(5) == ([0, 4, 2, 1], [[0, 1, 2], [4, 3, 2], [2, 1, 3], [1, 0, 2]], False)
    # c = 8 = P: the unragged answer (tests/test_pointcloud_gpu.py)
    assert _line(8) == ([0, 7, 3, 5], [[0, 1, 2], [7, 6, 5], [3, 2, 4], [5, 4, 6]], False)
    # c = 4 = n: every point is a centroid
    assert _line(4) == ([0, 3, 1, 2], [[0, 1, 2], [3, 2, 1], [1, 0, 2], [2, 1, 3]], False)
    # c = 3 < n: ids[3] = ids[0], its group with it
    assert _line(3) == ([0, 2, 1, 0], [[0, 1, 2], [2, 1, 0], [1, 0, 2], [0, 1, 2]], False)
    # c = 2 < k: the third slot repeats slot 0, the centroid itself
    assert _line(2) == ([0, 1, 0, 1], [[0, 1, 0], [1, 0, 1], [0, 1, 0], [1, 0, 1]], False)
    assert _line(1) == ([0] * 4, [[0] * 3] * 4, False)
    assert _line(0) == ([0] * 4, [[0] * 3] * 4, False)


def test_line_cloud_starts_and_faults():
    # start 1 of 5: the farthest is 4; then 0, 2, 3 tie at d = 1 -> 0; then 2, 3 tie -> 2
    assert _line(5, start=1)[0] == [1, 4, 0, 2]
    assert _line(5, start=1)[2] is False
    # a start not below the count: 0 and a fault; any start of an empty cloud
    assert _line(5, start=5) == (*_line(5)[:2], True)
    assert _line(5, start=-1) == (*_line(5)[:2], True)
    assert _line(0, start=0) == ([0] * 4, [[0] * 3] * 4, True)
    # counts outside [0, P]: clamped, a fault
    assert _line(9) == (*_line(8)[:2], True)
    assert _line(-1) == (*_line(0)[:2], True)


def test_equals_the_unragged_restatement_at_full_count():
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((2, 2, 40, 4)).astype(np.float32)
    start = rng.integers(0, 40, (2, 2)).astype(np.int32)
    counts = np.full((2, 2), 40, np.int32)
    for st in (None, start):
        ci, ni, fault = G.sample_group_counts(pts, 9, 5, counts, st)
        cr, nr = R.sample_group(pts, 9, 5, st)
        assert not fault
        np.testing.assert_array_equal(ci, cr)
        np.testing.assert_array_equal(ni, nr)
    np.testing.assert_array_equal(G.drawn_start_counts(11, 5, counts, 40, 3),
                                  R.drawn_start(11, 5, 2, 2, 40, 3))


def test_tail_rows_are_invisible_to_the_restatement():
    rng = np.random.default_rng(1)
    pts = rng.standard_normal((1, 1, 30, 3)).astype(np.float32)
    counts = np.array([[11]], np.int32)
    a = G.sample_group_counts(pts, 6, 4, counts)
    pts[0, 0, 11:] = np.nan
    b = G.sample_group_counts(pts, 6, 4, counts)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[0].max() < 11 and a[1].max() < 11


def test_selection_rule_brute_force():
    """All 1 <= P <= 64, 0 <= V <= 200: exactly min(V, P) slots, strictly increasing ranks, the
    first rank 0, every rank below V; and the kernel's per-pixel form names the same pixels."""
    for P in range(1, 65):
        for V in range(0, 201):
            ranks = G.selected_ranks(V, P)
            assert len(ranks) == min(V, P)
            if not ranks:
                continue
            assert ranks[0] == 0 and ranks[-1] < V
            assert all(a < b for a, b in zip(ranks, ranks[1:]))
            owners = {}
            for j in range(V):
                q = G.slot_of_rank(j, V, P)
                if q is not None:
                    assert q not in owners          # one writer per slot
                    owners[q] = j
            assert [owners[q] for q in range(len(ranks))] == ranks and len(owners) == len(ranks)


def test_selection_rule_fits_32_bits_at_the_limits():
    V, P = 1 << 20, 4096                              # j P and q V stay below 2^32
    assert (V - 1) * P < 1 << 32 and (P - 1) * V < 1 << 32
    for V, P in ((1 << 20, 4096), ((1 << 20) - 1, 4095), (307200, 1024), (4097, 4096)):
        ranks = G.selected_ranks(V, P)
        for q in (0, 1, P // 2, P - 2, P - 1):
            assert G.slot_of_rank(ranks[q], V, P) == q
        assert ranks[-1] < V


def test_pack_counts_restatement():
    counts = np.array([[3, 6], [4, 5], [5, 7]], np.int32)
    w, fault = G.pack_counts(None, 5, 1 << 4, counts, [1, 2], [4, 6])
    assert w.tolist() == [0b11101, 0b11011, 0b11111] and not fault
    mask = np.ones((3, 5), bool)
    mask[2, 1] = mask[0, 0] = mask[1, 4] = False       # a Readout set flagged absent: sample 1
    w, fault = G.pack_counts(mask, 5, 1 << 4, counts, [1, 2], [4, 6])
    assert w.tolist() == [0b11100, 0b11011, 0b11101] and fault


def test_unproject_restatement_known_answer():
    depth = np.zeros((1, 1, 2, 4), np.uint16)
    depth[0, 0, 0, 1], depth[0, 0, 1, 2], depth[0, 0, 1, 3] = 1000, 2000, 5000   # 5 m: too far
    intr = np.array([[[2.0, 4.0, 1.0, 0.0]]], np.float32)
    pts, cnt = G.unproject(depth, intr, 3, scale=0.001)
    assert cnt.tolist() == [[2]]
    z1, z2 = np.float32(1000) * np.float32(0.001), np.float32(2000) * np.float32(0.001)
    np.testing.assert_array_equal(pts[0, 0], np.array(
        [[0.0, 0.0, z1], [(np.float32(1.0) * z2) / np.float32(2.0), z2 / np.float32(4.0), z2],
         [0, 0, 0]], np.float32))


def test_python_surface_takes_the_new_arguments():
    """Signatures only (no device): counts / point_cloud_counts reach every public function."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    from multi_modal_transformers_tokenmerge_amd.tokenizers.pointclouds import depth_to_point_cloud
    from multi_modal_transformers_tokenmerge_amd.tokenizers.pointclouds.point_cloud_tokenizer \
        import PointCloudTokenizer as T
    assert "counts" in inspect.signature(K.pc_sample_group).parameters
    for fn in (T.forward, T.sample_and_group, T.farthest_point_sampling, T.__call__):
        assert "counts" in inspect.signature(fn).parameters, fn
    m = O.Octo
    for fn in (m.generate_readouts, m.compute_diffusion_denoise_loss, m.compute_l2_loss,
               m.compute_ce_loss, m.predict_diffusion_denoise_term, m.predict_diffusion_action,
               m.predict_continuous_action, m.predict_action_logits,
               m.predict_categorical_action, O._step_kw, O.continuous_train_step,
               O.categorical_train_step, O.diffusion_train_step, DDPStep.__init__):
        assert "point_cloud_counts" in inspect.signature(fn).parameters, fn
    assert list(inspect.signature(depth_to_point_cloud).parameters) == \
        ["depth", "intrinsics", "num_points", "depth_scale", "z_range", "pose", "rgb"]
    assert O._step_kw(None, None, point_cloud_counts=7) == {"point_cloud_counts": 7}
    with pytest.raises(ValueError):
        depth_to_point_cloud(np.zeros((4, 8)), None, 4)      # not a tensor
