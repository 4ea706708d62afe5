"""dg_elev_hist and dg_beam_project (csrc/beam_project.hip) against tests/beam_ref.py.  Everything is exact: integer counts,
cell indices, records copied bit for bit.  tests/test_beams_cpu.py holds the clouds used here to have no point within 1e-9 rad
of a bin edge or of a midpoint between two beams and none inside the column band, so nothing is excluded."""
import ctypes

import numpy as np
import pytest
import torch

from tests import beam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, HI = -np.pi / 2, np.pi / 2


@pytest.fixture(scope="module")
def raw():
    from dusty_gan_amd import _lib
    _lib.lib()
    from dusty_gan_amd.datasets import raw as M
    return M


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cat(clouds):
    return np.concatenate(clouds).astype(np.float32), np.concatenate([[0], np.cumsum([len(c) for c in clouds])])


def _project(raw, clouds, beams, W):
    pts, offs = _cat(clouds)
    out, cells = raw.project_clouds_beams(torch.from_numpy(pts), offs, beams, W=W, return_cells=True)
    return out.cpu().numpy(), cells.cpu().numpy().astype(np.int64), offs


# ------------------------------------------------------------------------------------------------ dg_elev_hist
@pytest.mark.parametrize("NB", [64, 8192, 16384])   # 16384: the contract's upper limit, 64 KB of LDS
@pytest.mark.parametrize("lo,hi", [(LO, HI), (-0.4, 0.1)])
def test_histogram_equals_the_reference(NB, lo, hi):
    """S = 3 clouds of 0, 700 and 5000 points: points at and beyond both depth limits, outside [lo, hi), non-finite and at
    the origin; one call over all clouds equals two calls over a split of them"""
    from dusty_gan_amd.datasets.beams import elevation_histogram
    clouds = R.hist_clouds()
    pts, offs = _cat(clouds)
    want = R.histogram(pts, 1.0, 120.0, lo, hi, NB)
    assert 0 < want.sum() < len(pts) and ((want > 0).sum() > NB // 2 or NB > 5000)
    got = elevation_histogram((torch.from_numpy(pts), offs), 1.0, 120.0, lo, hi, NB)
    assert got.dtype == np.int64 and got.shape == (NB,)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    a = elevation_histogram((pts[:offs[2]], offs[:3]), 1.0, 120.0, lo, hi, NB)
    b = elevation_histogram(torch.from_numpy(pts[offs[2]:]).to(DEV), 1.0, 120.0, lo, hi, NB)
    assert np.array_equal(a + b, want)


def test_histogram_arguments():
    from dusty_gan_amd import _lib as L
    pts = torch.zeros(8, 4, device=DEV)
    offs = torch.tensor([0, 8], device=DEV)
    hist = torch.zeros(64, dtype=torch.int64, device=DEV)

    def call(p=pts, o=offs, S=1, lo=LO, hi=HI, NB=64, h=hist):
        return L.lib().dg_elev_hist(L.ptr(p), L.ptr(o), S, 0.9, 120.0, lo, hi, NB, L.ptr(h), L.stream_ptr())
    assert call() == L.DG_OK
    for kw in (dict(p=None), dict(o=None), dict(h=None), dict(lo=0.5, hi=0.5), dict(lo=0.5, hi=-0.5), dict(NB=63),
               dict(NB=16385), dict(S=0)):
        assert call(**kw) == L.DG_EINVAL, kw
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0


# ------------------------------------------------------------------------------------------------ dg_beam_project
@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_projection_equals_the_reference_cell_for_cell(raw, name):
    beams, W, clouds = R.gpu_case(name)
    got, cells, offs = _project(raw, clouds, beams, W)
    assert got.shape == (len(clouds), len(beams), W, 4) and got.dtype == np.float32
    for s, pts in enumerate(clouds):
        want, want_cell = R.project(pts, beams, W)
        assert np.array_equal(cells[offs[s]:offs[s + 1]], want_cell), s
        assert np.array_equal(_bits(got[s]), _bits(want)), (s, np.argwhere((_bits(got[s]) != _bits(want)).any(-1))[:10])
    # bit-identical from run to run, and whatever S is: every cloud alone gives its image of the batch
    again, _, _ = _project(raw, clouds, beams, W)
    assert np.array_equal(_bits(again), _bits(got))
    if len(clouds) > 1:
        alone, _, _ = _project(raw, clouds[1:2], beams, W)
        assert np.array_equal(_bits(alone[0]), _bits(got[1]))


def _ray(W, column, r, z, refl):
    yaw = -np.pi + (W - 1 - column + 0.5) * (2 * np.pi / W)   # the middle of `column`
    return [r * np.cos(yaw), r * np.sin(yaw), z, refl]


def test_ties_non_finite_points_and_an_empty_scan(raw):
    a, W = 0.1, 8
    beams = np.array([a, -a])
    up, down = 10.0 * np.tan(a), -10.0 * np.tan(a)
    tie = np.array([_ray(W, 5, 10.0, down, 1.0), _ray(W, 5, 10.0, down, 2.0),        # equal float32 range, one cell
                    _ray(W, 2, 10.0, 0.0, 3.0),                                     # z = 0 between the beams at +-a
                    _ray(W, 3, 10.0, up, 4.0), _ray(W, 3, 7.0, 7.0 * np.tan(a), 5.0),   # the nearer point wins, whatever its index
                    [np.nan, 1, 1, 6], [1, np.inf, 1, 7], [0, 0, 0, 8]], dtype=np.float32)
    empty = np.zeros((0, 4), np.float32)
    got, cells, offs = _project(raw, [tie, empty, tie[::-1].copy()], beams, W)
    want, want_cell = R.project(tie, beams, W)
    assert want_cell.tolist() == [W + 5, W + 5, 2, 3, 3, -1, -1, -1]
    assert np.array_equal(cells[:8], want_cell) and np.array_equal(_bits(got[0]), _bits(want))
    assert got[0, 1, 5, 3] == 1.0 and got[0, 0, 2, 3] == 3.0 and got[0, 0, 3, 3] == 5.0
    assert (got[0] != 0).any(-1).sum() == 3
    assert not got[1].any()                                                         # the empty scan: an all-zero image
    assert got[2, 1, 5, 3] == 2.0                                                   # reversed: the other record has the lower index
    assert np.array_equal(_bits(got[2]), _bits(R.project(tie[::-1], beams, W)[0]))


def test_permutation_and_round_trip(raw):
    """a permutation of a tie-free scan gives the same image; an ordered scan with one point per cell, shuffled, comes back"""
    beams, W, clouds = R.gpu_case("32x64")
    pts = clouds[0]
    _, cell = R.project(pts, beams, W)
    d32 = R.range64(pts).astype(np.float32)
    assert len(set(zip(cell.tolist(), d32.tolist()))) == len(pts)                    # tie-free
    rng = np.random.default_rng(5)
    got, _, _ = _project(raw, [pts, pts[rng.permutation(len(pts))], pts[::-1].copy()], beams, W)
    assert np.array_equal(_bits(got[1]), _bits(got[0])) and np.array_equal(_bits(got[2]), _bits(got[0]))
    H = 32
    ordered = R.synthetic_sensor(beams, W, seed=77, jitter=0.002, shuffle=False)
    assert ordered.shape == (H * W, 4)
    image, cell = R.project(ordered, beams, W)
    assert sorted(cell.tolist()) == list(range(H * W))                              # one point per cell
    back, _, _ = _project(raw, [ordered[rng.permutation(H * W)]], beams, W)
    assert np.array_equal(_bits(back[0]), _bits(image))
    # the file's beam-major order is the image's rows; its azimuth steps run against the columns
    assert np.array_equal(_bits(back[0]), _bits(ordered.reshape(H, W, 4)[:, ::-1]))


def test_projection_arguments(raw):
    from dusty_gan_amd import _lib as L
    pts = torch.ones(8, 4, device=DEV)
    offs = torch.tensor([0, 8], device=DEV)
    keys = torch.empty(256 * 64, dtype=torch.int64, device=DEV)
    out = torch.empty(256 * 64 * 4, device=DEV)

    def call(p=pts, o=offs, S=1, beams=(0.1, 0.0, -0.1), H=None, W=16, k=keys, o_=out, no_table=False):
        b = (ctypes.c_double * max(len(beams), 1))(*beams)
        return L.lib().dg_beam_project(L.ptr(p), L.ptr(o), S, None if no_table else b, len(beams) if H is None else H, W,
                                       L.ptr(k), None, L.ptr(o_), L.stream_ptr())
    assert call() == L.DG_OK
    for kw in (dict(H=0), dict(W=8193), dict(W=0), dict(beams=(0.0, 0.1)), dict(beams=(0.1, 0.1)), dict(beams=(0.1, float("nan"))),
               dict(p=None), dict(o=None), dict(k=None), dict(o_=None), dict(no_table=True), dict(S=0),
               dict(beams=tuple(np.linspace(1, -1, 257)))):
        assert call(**kw) == L.DG_EINVAL, kw
    assert call(beams=tuple(np.linspace(1, -1, 256)), W=64) == L.DG_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        raw.project_clouds_beams(pts, [0, 8], [0.0, 0.1], W=16)
    with pytest.raises(RuntimeError if not torch.cuda.is_available() else AssertionError):
        raw.project_clouds_beams(torch.ones(8, 3), [0, 8], [0.1, 0.0], W=16)
