"""Directed tests of the encoder's corner colour streams (yk_corners.hip: yk_corner_owner_body, yk_corner_stream_body, the scan, and their batch forms
in yk_streams_batch.hip) on images that set the tile bitmaps of all seven passes on purpose (tests/corner_cases.py; tests/test_corner_cases.py
shows from the oracle and a sequential model alone that every case holds what it claims).  Every comparison is byte for byte.

What the cases pin: every value of a bitmap byte in every pass, with the same-byte filter's four relations alone, together and at the two places
where a byte of the 16-wide passes wraps; every pair of passes as neighbours in every placement, the later pass first in bit order where the
geometry allows; neighbours across bytes, swizzle blocks and workgroups; workgroups that own 0 .. 4 colours at every run offset mod 4 (head, whole
words, tail of the copy-out); 8192 colours in a workgroup (the last count on the LDS path), 8383 (direct stores) and two direct-store workgroups
in a row; clamped reads of the last lattice column and row, partial swizzle blocks, an image without a tile, a half-used bitmap word; the stripe
edge index; a handle reused from dense to sparse to empty; batches of three with a dense, an empty and a sparse frame; two row stripes merged.
A mismatch names the pass, the first differing colour, its workgroup and run, the owning tile and its bitmap byte."""
import numpy as np
import pytest

from tests import corner_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hip_batch():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


def _encode(e, c):
    e.set_image(c["planes"])
    e.encode(3, False, False)


def _same_streams(streams, name, what):
    """the seven streams against the oracle and against the model; the story comes from the model's census"""
    c, m = cc.case(name), cc.model(name)
    for p in range(7):
        got, want = np.asarray(streams[p]), c["run"][p][2]
        assert got.size == want.size and np.array_equal(got, want), (what, name, "against the oracle", cc.story(name, p, got))
        assert np.array_equal(got, m["streams"][p]), (what, name, "against the model", cc.story(name, p, got))


def _same_bitmaps(e, name, what):
    c = cc.case(name)
    for p in range(7):
        got, want = e.gradient_bitmap(p), c["run"][p][1]
        assert got.size == want.size and np.array_equal(got, want), (what, name, "bitmap of pass", p, "first differing byte", int(np.flatnonzero(got != want)[0]) if got.size == want.size else -1)
    assert e.gradient_counts().tolist() == [cnt for cnt, _, _ in c["run"]], (what, name, "counts")


def _same_edges(e, name, what):
    """both key rows are the model's owner keys; an owned point's index is its colour's ordinal in its pass; the others read 0xFFFFFFFF"""
    m = cc.model(name)
    keys, idx = e.gradient_corner_edges()
    for row, ly in ((0, 0), (1, m["owner"].shape[0] - 1)):
        want_keys = m["owner"][ly]
        assert np.array_equal(keys[row], want_keys), (what, name, "owner keys of lattice row", ly, "first at x =", int(np.flatnonzero(keys[row] != want_keys)[0]))
        want_idx = np.where(want_keys != cc.NONE, m["ordinal"][ly], cc.NONE).astype(np.uint32)
        assert np.array_equal(idx[row], want_idx), (what, name, "edge index of lattice row", ly, "first at x =", int(np.flatnonzero(idx[row] != want_idx)[0]))


# ---- every case on one handle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_against_the_oracle_and_the_model(hip, oracle_built, name):
    _encode(hip, cc.case(name))
    _same_bitmaps(hip, name, "one handle")
    _same_streams([hip.gradient_corners(p) for p in range(7)], name, "one handle")


@pytest.mark.parametrize("name", cc.WHOLE_IMAGE_EDGE_NAMES)
def test_edge_index(hip, oracle_built, name):
    _encode(hip, cc.case(name))
    _same_edges(hip, name, "edge index")
    _same_streams([hip.gradient_corners(p) for p in range(7)], name, "after the edge index")


# ---- stale state -------------------------------------------------------------------------------------------------------------------------------------
def test_dense_then_sparse_then_empty_on_one_handle(oracle_built):
    """perThread, the lattice owners, edgeIdx, the pending totals and the padding clear: nothing of the denser image before survives"""
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    try:
        for step, name in enumerate(cc.STALE):
            _encode(e, cc.case(name))
            got = [e.gradient_corners(p) for p in range(7)]
            _same_streams(got, name, ("reused handle, step", step))
            _same_edges(e, name, ("reused handle, step", step))
            fresh = HipTileEncoder(0)
            try:
                _encode(fresh, cc.case(name))
                for p in range(7):
                    assert np.array_equal(fresh.gradient_corners(p), got[p]), (name, "fresh handle, pass", p)
                fk, fi = fresh.gradient_corner_edges()
                rk, ri = e.gradient_corner_edges()
                assert np.array_equal(fk, rk) and np.array_equal(fi, ri), (name, "edges of a fresh handle")
            finally:
                fresh.close()
        name = cc.STALE[-1]
        for turn in range(2):
            e.gradient_corners_run()
            _same_streams([e.gradient_corners(p) for p in range(7)], name, ("gradient_corners_run", turn))
            _same_edges(e, name, ("gradient_corners_run", turn))
        # and back up: the dense image after the empty one
        _encode(e, cc.case(cc.STALE[0]))
        e.gradient_corners_run()
        _same_streams([e.gradient_corners(p) for p in range(7)], cc.STALE[0], "dense after empty")
    finally:
        e.close()


# ---- batches -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bname", sorted(cc.BATCHES))
def test_batch_of_three(hip_batch, oracle_built, bname):
    """the frame-strided kernels: a dense, an empty and a sparse frame of one shape; every frame against its own oracle run, the model, and the
    single-image path on the selected frame"""
    import torch
    names = cc.BATCHES[bname]
    frames = torch.from_numpy(np.ascontiguousarray(np.stack([cc.case(n)["planes"] for n in names]))).cuda()
    e = hip_batch
    e.set_batch(frames)
    e.encode_batch(3, False)
    rows = e.streams_batch(corners=True, range1d=False)
    assert len(rows) == 3
    for f, (row, name) in enumerate(zip(rows, names)):
        want = cc.case(name)["run"]
        assert list(row.rgb_bytes) == [rgb.size for _, _, rgb in want], (bname, "frame", f, name, "stream lengths", list(row.rgb_bytes))
        _same_streams(row.download()["rgb"], name, (bname, "frame", f))
    for f, name in enumerate(names):
        e.select_frame(f)
        _same_bitmaps(e, name, (bname, "selected frame", f))
        _same_streams([e.gradient_corners(p) for p in range(7)], name, (bname, "selected frame", f))
    rows2 = e.streams_batch(corners=True, range1d=False)                        # again, after the single-image path ran on every frame
    for f, (row, name) in enumerate(zip(rows2, names)):
        _same_streams(row.download()["rgb"], name, (bname, "frame", f, "again"))


# ---- stripes -----------------------------------------------------------------------------------------------------------------------------------------
def test_two_row_stripes_merge_to_the_whole_image(oracle_built):
    from yaik_amd import distributed as ykd
    from yaik_amd.encoder import HipTileEncoder
    name = "mosaic_256_a"
    c = cc.case(name)
    H = c["h"]
    streams, edges = [], []
    for r in range(2):
        y0, h, halo = ykd.stripe_rows(H, 2, r)
        assert h == 128 and halo == 1 - r
        e = HipTileEncoder(0)
        try:
            e.set_image(np.ascontiguousarray(c["planes"][:, y0:y0 + h + halo, :]), full_h=H, y0=y0, halo_rows=halo)
            e.encode(3, False, False)
            streams.append([e.gradient_corners(p) for p in range(7)])
            edges.append(e.gradient_corner_edges())
        finally:
            e.close()
    shared = (edges[0][0][1] != cc.NONE) & (edges[1][0][0] != cc.NONE)
    assert shared.sum() > 8, "both stripes emit points of the shared lattice row"
    _same_streams(ykd.merge_corner_streams(streams, edges), name, "two stripes merged")
