"""The row map of Hiera's padded windows (csrc/flash.hip s2h_window_map, ops.window_map_host) against a
numpy zero-pad + partition of the token-id image.  Host only: the table is built and range-checked by
the library on the CPU; the kernels that read it are covered by test_hiera_win_map_gpu.py."""
import numpy as np
import pytest

GEOMS = [(16, 16, 14), (32, 32, 14), (20, 17, 14), (14, 14, 14)]


def _ops():
    from sam2_video.kernels import ops
    return ops


def _partition(img, ws, fill):
    """numpy window partition of a 2-D image padded (bottom / right) with `fill`: [nW, ws * ws]"""
    H, W = img.shape
    nh, nw = -(-H // ws), -(-W // ws)
    pad = np.full((nh * ws, nw * ws), fill, dtype=img.dtype)
    pad[:H, :W] = img
    return pad.reshape(nh, ws, nw, ws).transpose(0, 2, 1, 3).reshape(nh * nw, ws * ws)


@pytest.mark.parametrize("H,W,ws", GEOMS)
def test_row_map_is_the_partition_of_the_padded_id_image(H, W, ws):
    row, padidx, sets = _ops().window_map_host(H, W, ws)
    ids = np.arange(H * W, dtype=np.int32).reshape(H, W)
    want = _partition(ids, ws, -1)
    assert row.dtype == np.int32 and row.shape == want.shape
    # padded positions are exactly the -1 entries; every other entry is the token at that position
    assert np.array_equal(row, want)
    assert np.array_equal(row < 0, want == -1)
    # gathering any per-token payload through the map equals partitioning its zero-padded image
    payload = (np.arange(H * W, dtype=np.int64) * 7 + 3).reshape(H, W)
    got = np.where(row >= 0, payload.ravel()[np.maximum(row, 0)], 0)
    assert np.array_equal(got, _partition(payload, ws, 0))
    # each token once, every entry -1 or within [0, H W)
    real = row[row >= 0]
    assert real.min() == 0 and real.max() == H * W - 1 and np.array_equal(np.sort(real), np.arange(H * W))
    assert ((row == -1) | ((row >= 0) & (row < H * W))).all()


@pytest.mark.parametrize("H,W,ws", GEOMS)
def test_padded_rows_are_numbered_in_the_column_sum_order(H, W, ws):
    """padidx = the padded position's index in window_pad_colsum's enumeration of an image: the rows
    y >= H (all x of the padded width), then the rows y < H with x >= W"""
    row, padidx, sets = _ops().window_map_host(H, W, ws)
    nh, nw = -(-H // ws), -(-W // ws)
    Hp, Wp = nh * ws, nw * ws
    order = np.full((Hp, Wp), -1, dtype=np.int32)
    n = 0
    for y in range(H, Hp):
        for x in range(Wp):
            order[y, x] = n
            n += 1
    for y in range(H):
        for x in range(W, Wp):
            order[y, x] = n
            n += 1
    assert n == Hp * Wp - H * W
    want = order.reshape(nh, ws, nw, ws).transpose(0, 2, 1, 3).reshape(nh * nw, ws * ws)
    assert np.array_equal(padidx, want)
    assert np.array_equal(padidx >= 0, row < 0)
    # 16-row sets that hold a real token
    for wn in range(nh * nw):
        m = 0
        for s in range(-(-ws * ws // 16)):
            if (row[wn, 16 * s:16 * s + 16] >= 0).any():
                m |= 1 << s
        assert int(sets[wn]) & 0xFFFFFFFF == m


def test_small_geometry_has_every_window_kind():
    """(16, 16, 14): full, right-partial, bottom-partial and corner windows with 196, 28, 28, 4 real rows"""
    row, _, _ = _ops().window_map_host(16, 16, 14)
    assert [(r >= 0).sum() for r in row] == [196, 28, 28, 4]
    row, _, _ = _ops().window_map_host(14, 14, 14)
    assert row.shape == (1, 196) and (row >= 0).all()


def test_domain_of_the_mode():
    from sam2_video.kernels import _lib
    ok = _lib.lib().s2h_flash_win_ok
    assert ok(1, 8, 32, 32, 14, 8, 56) == 1      # the bench geometry, bf16
    assert ok(1, 32, 16, 16, 14, 2, 72) == 1     # the 128-wide image
    assert ok(1, 2, 32, 32, 14, 8, 56) == 0      # 144 batch-heads: the partitioned dQ launch splits its keys
    assert ok(0, 8, 32, 32, 14, 8, 56) == 0      # fp32 compute
    assert ok(1, 8, 16, 16, 7, 8, 112) == 0      # 49-position windows: not the flash domain
    assert ok(1, 8, 32, 32, 14, 8, 60) == 0      # rows not 16-B aligned
    assert ok(1, 8, 32, 32, 23, 8, 56) == 0      # more positions than the kernels' map holds
    assert ok(1, 1, 4096, 4096, 14, 8, 56) == 0  # an image past the 32-bit offsets
    with pytest.raises(Exception):
        _ops().window_map_host(32, 32, 23)
