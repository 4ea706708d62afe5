"""The object-removal kernels (csrc/object_removal.hip through dusty_gan_amd/removal.py) against tests/label_util.py.
Integer work and bit-for-bit copies: every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import label_util as LU

pytestmark = pytest.mark.gpu

SHAPES = [(4, 8), (5, 70), (64, 256)]    # 5 x 70: a row crosses a wave, W no multiple of 64


@pytest.fixture(scope="module")
def RM():
    from dusty_gan_amd import _lib
    _lib.lib()
    from dusty_gan_amd import removal
    return removal


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("shape", [((64, 2048), (64, 512)), ((8, 32), (4, 8)), ((5, 7), (3, 11))])
def test_label_resize(RM, shape):
    (Hs, Ws), (H, W) = shape
    rng = np.random.default_rng(Hs * Ws)
    sem = rng.integers(0, 20, (2, Hs, Ws)).astype(np.uint8)
    got = RM.label_resize(_dev(sem), H, W).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, LU.label_resize(sem, H, W))
    # the cells torch's legacy nearest picks (what the dataset's transform resamples the scan with)
    want = torch.nn.functional.interpolate(torch.from_numpy(sem)[:, None].float(), size=(H, W), mode="nearest")[:, 0]
    assert np.array_equal(got, want.numpy().astype(np.uint8))


def _scene(rng, B, H, W, kind):
    """(sem, valid, table): classes 1 and 6 are removed; flagged pixels on both seam columns and on both edge rows"""
    sem = rng.integers(7, 20, (B, H, W)).astype(np.uint8)
    valid = (rng.random((B, H, W)) < 0.8).astype(np.float32)
    table = np.zeros(256, dtype=np.uint8)
    table[[1, 6]] = 1
    if kind == "all":
        sem[:], valid[:] = 1, 1
    elif kind == "some":
        for b in range(B):
            for h, w, c in ((0, 0, 1), (H - 1, W - 1, 6), (H // 2, W // 2, 1), (0, W - 1, 6), (H - 1, 0, 1)):
                sem[b, h, w], valid[b, h, w] = c, 1
            sem[b, H // 2, (W // 2 + 3) % W], valid[b, H // 2, (W // 2 + 3) % W] = 1, 0     # an object pixel that is not measured
            k = rng.integers(0, H * W, max(1, H * W // 50))
            sem[b].reshape(-1)[k] = 6
    return sem, valid, table


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("r", [0, 1, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_remove_mask(RM, shape, r, B):
    H, W = shape
    for kind in ("some", "all", "none"):
        rng = np.random.default_rng(H * 1000 + W + r)
        sem, valid, table = _scene(rng, B, H, W, kind)
        want, want_counts = LU.remove_mask(sem, valid, table, r)
        remove, counts = RM.remove_mask(_dev(sem), _dev(valid)[:, None], _dev(table), r)
        assert remove.dtype == torch.uint8 and tuple(remove.shape) == (B, H, W)
        assert np.array_equal(remove.cpu().numpy(), want), (kind, np.argwhere(remove.cpu().numpy() != want)[:8])
        assert np.array_equal(counts.cpu().numpy().astype(np.uint32), want_counts)
        for b in range(B):
            assert np.array_equal(want_counts[b], np.bincount(sem[b][valid[b] != 0], minlength=256))
        if kind == "all":
            assert want.all()
        if kind == "none":
            assert not want.any()
        if kind == "some":
            assert want.any() and (r == 8 or H * W < 256 or not want.all())
            if r == 0:
                assert np.array_equal(want != 0, (valid != 0) & (table[sem] != 0))


def test_remove_mask_arguments(RM):
    sem = torch.zeros(1, 4, 8, dtype=torch.uint8, device="cuda")
    valid = torch.ones(1, 4, 8, device="cuda")
    table = RM.class_table([1], "cuda")
    for r in (-1, 9):
        with pytest.raises(ValueError, match="dilate"):
            RM.remove_mask(sem, valid, table, r)
    from dusty_gan_amd import _lib as L
    out = torch.empty_like(sem)
    cp = torch.zeros(1, 256, dtype=torch.int32, device="cuda")
    assert L.lib().dg_remove_mask(L.ptr(sem), L.ptr(valid), L.ptr(table), 1, 4, 8, 9, L.ptr(out), L.ptr(cp), L.stream_ptr()) == L.DG_EINVAL


@pytest.mark.parametrize("keep_is_depth", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_compose(RM, shape, B, keep_is_depth):
    H, W = shape
    rng = np.random.default_rng(H * W + B)
    sem = rng.integers(0, 20, (B, H, W)).astype(np.uint8)
    valid = (rng.random((B, H, W)) < 0.5).astype(np.float32)
    remove = (rng.random((B, H, W)) < 0.5).astype(np.uint8)
    tgt = rng.random((B, H, W)).astype(np.float32)
    gen = rng.random((B, H, W)).astype(np.float32)
    gen.reshape(-1)[::7] = tgt.reshape(-1)[::7]                     # equal depths: not in front
    tol = 0.25 if keep_is_depth else 0.0
    keep = gen.copy() if keep_is_depth else (rng.random((B, H, W)) < 0.6).astype(np.float32)
    if keep_is_depth:
        keep.reshape(-1)[::5] = np.float32(tol)                     # exactly at the tolerance: not kept
    for v in (0, 1):
        for r in (0, 1):
            assert ((valid == v) & (remove == r)).any()
    want = LU.compose(tgt, valid, gen, keep, keep_is_depth, tol, remove, sem, 3)
    got = RM.compose(_dev(tgt)[:, None], _dev(valid)[:, None], _dev(gen)[:, None], _dev(keep)[:, None], _dev(remove), _dev(sem),
                     keep_is_depth=keep_is_depth, tol=tol, fill_label=3)
    inv_out, source, sem_out, counts = (t.cpu().numpy() for t in got)
    assert inv_out.shape == (B, 1, H, W) and inv_out.dtype == np.float32
    assert np.array_equal(inv_out[:, 0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(source, want[1]) and np.array_equal(sem_out, want[2])
    assert np.array_equal(counts, want[3]), (counts, want[3])
    # bit-equal to the selected input, and the counts from the maps
    assert np.array_equal(inv_out[:, 0].view(np.uint32)[source == 1], tgt.view(np.uint32)[source == 1])
    assert np.array_equal(inv_out[:, 0].view(np.uint32)[source == 2], gen.view(np.uint32)[source == 2])
    assert not inv_out[:, 0].view(np.uint32)[source == 0].any()
    assert np.array_equal(counts[:, 1], (source == 2).reshape(B, -1).sum(1)) and (H * W < 256 or (counts[:, 2] > 0).all())
    assert set(np.unique(source)) == {0, 1, 2}


def _cloud_case(rng, B, N, stride, H, W, counts, mode):
    rec = rng.normal(size=(B, N, stride)).astype(np.float32)
    rec.view(np.uint32)[:, ::11, 0] = 0x7FC00001                       # a NaN payload must survive as it is
    idx = rng.integers(0, H * W, (B, N)).astype(np.int32)
    idx[:, ::9] = -1                                                   # took no part: stays
    labels = rng.integers(0, 2 ** 32, (B, N), dtype=np.uint64).astype(np.uint32)
    remove = {"mixed": (rng.random((B, H, W)) < 0.4), "all": np.zeros((B, H, W), bool), "none": np.ones((B, H, W), bool)}[mode]
    return rec, idx, labels, remove.astype(np.uint8), np.asarray(counts, dtype=np.int32)


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 5000])
def test_cloud_remove(RM, N, stride):
    H, W, B = 8, 32, 3
    rng = np.random.default_rng(N * 10 + stride)
    for mode in ("mixed", "all", "none"):          # "all": keep everything; "none": keep nothing but the idx = -1 records
        rec, idx, labels, remove, counts = _cloud_case(rng, B, N, stride, H, W, [N, 0, max(N - 3, 0) // 2 + (N > 1)], mode)
        want = LU.cloud_remove(rec, counts, idx, remove, labels)
        args = (_dev(rec), _dev(counts), _dev(idx), _dev(remove), _dev(labels.view(np.int32)))
        out = RM.cloud_remove(*args)
        again = RM.cloud_remove(*args)
        o_rec, o_lab, o_idx, o_cnt = (t.cpu().numpy() for t in out)
        assert o_rec.shape == (B, N, 4) and o_cnt.tolist() == [len(w[0]) for w in want], (mode, o_cnt)
        for b in range(B):
            k = int(o_cnt[b])
            assert np.array_equal(o_rec[b, :k].view(np.uint32), want[b][0]), (mode, b)
            assert np.array_equal(o_lab[b, :k].view(np.uint32), want[b][1]) and np.array_equal(o_idx[b, :k], want[b][2])
            for t, u in zip(out[:3], again[:3]):   # two calls, identical bytes
                assert torch.equal(t[b, :k].view(torch.int32) if t.dtype == torch.float32 else t[b, :k],
                                   u[b, :k].view(torch.int32) if u.dtype == torch.float32 else u[b, :k])
        assert torch.equal(out[3], again[3])
        assert o_cnt[1] == 0
        if mode == "all":
            assert o_cnt[0] == N
        if mode == "none":
            assert o_cnt[0] == len(range(0, N, 9))
    # without counts and without labels
    rec, idx, labels, remove, _ = _cloud_case(rng, 2, N, stride, H, W, [N, N], "mixed")
    want = LU.cloud_remove(rec, [N, N], idx, remove, labels)
    o_rec, o_lab, o_idx, o_cnt = RM.cloud_remove(_dev(rec), None, _dev(idx), _dev(remove))
    assert o_lab is None and o_cnt.tolist() == [len(w[0]) for w in want]
    for b in range(2):
        assert np.array_equal(o_rec[b, :int(o_cnt[b])].cpu().numpy().view(np.uint32), want[b][0])
