"""Host side of the batch sampler's kernels (include/parc_mdm_batch.h): the per-clip terrain / cell-list tables and the draw table as
the plain arrays the entry points read.  numpy and ctypes only, so the host build of the kernels (tests) packs its inputs here too."""
import ctypes

import numpy as np

from .. import _hip_mdm_batch as mb


def pack_clip_tables(terrains, mask_lists):
    """terrains: per clip (hf [X, Y], hf_maxmin [X, Y, 2], min_point [2], dxdy [2]) as numpy; mask_lists: per clip the per-frame [k, 2]
    integer arrays.  -> (clips: MdmClipS array, pool float32, cell_start int32, cells int32, mask_cells)
    pool holds every clip's heights, then its band interleaved (maximum, minimum); cell_start holds num_frames + 1 running offsets per
    clip, cells the flat indices i * dim_y + j."""
    n = len(terrains)
    clips = (mb.MdmClipS * max(n, 1))()
    parts, off, starts, cells, row, n_cells, mask_cells = [], 0, [], [], 0, 0, 1
    for k, ((hf, band, mp, dxdy), lists) in enumerate(zip(terrains, mask_lists)):
        hf = np.ascontiguousarray(hf, np.float32)
        band = np.ascontiguousarray(band, np.float32)
        X, Y = hf.shape
        assert band.shape == (X, Y, 2)
        e = clips[k]
        e.off_hf, e.off_band, e.dim_x, e.dim_y = off, off + X * Y, X, Y
        e.min_x, e.min_y, e.dx, e.dy = float(mp[0]), float(mp[1]), float(dxdy[0]), float(dxdy[1])
        e.frame_off, e.num_frames = row, len(lists)
        parts += [hf.reshape(-1), band.reshape(-1)]
        off += 3 * X * Y
        counts = [len(a) for a in lists]
        starts.append(n_cells + np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
        for a in lists:
            a = np.asarray(a, np.int64).reshape(-1, 2)
            cells.append(a[:, 0] * Y + a[:, 1])
        row += len(lists) + 1
        n_cells += int(sum(counts))
        mask_cells = max(mask_cells, X * Y)
    assert off < 2 ** 31 and n_cells < 2 ** 31
    pool = np.concatenate(parts).astype(np.float32) if parts else np.zeros(1, np.float32)
    cell_start = np.concatenate(starts).astype(np.int32) if starts else np.zeros(1, np.int32)
    cells = np.concatenate(cells).astype(np.int32) if cells else np.zeros(0, np.int32)
    if cells.size == 0:
        cells = np.zeros(1, np.int32)           # never read: every range is empty
    return clips, pool, cell_start, cells, mask_cells


def pack_draws(change_height, new_height, pool_kind, pool_radius, num_boxes, boxes, max_boxes):
    """-> one uint8 array: n parc_mdm_draw_t rows, then n * max_boxes parc_mdm_box_t rows (one host-to-device copy carries both);
    returns (bytes array, offset of the box table)"""
    n = len(change_height)
    d = np.zeros((n, 9), np.int32)
    d[:, 0] = change_height
    d[:, 1] = np.asarray(new_height, np.float32).view(np.int32)
    d[:, 2:5] = pool_kind
    d[:, 5:8] = pool_radius
    d[:, 8] = num_boxes
    assert ctypes.sizeof(mb.MdmDrawS) == 36 and ctypes.sizeof(mb.MdmBoxS) == 24
    b = np.ascontiguousarray(boxes, np.float32).reshape(n, max_boxes, 6) if max_boxes else np.zeros((n, 0, 6), np.float32)
    raw = np.concatenate([d.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)])
    return raw, n * 36


def make_cfg(seq_len, ref_idx, num_x_neg, num_y_neg, dim_x, dim_y, z_style, mode, max_boxes, fps, max_h):
    return mb.MdmCfgS(seq_len, ref_idx, num_x_neg, num_y_neg, dim_x, dim_y, z_style, mode, max_boxes, float(np.float32(1.0 / fps)),
                      float(np.float32(-max_h)), float(np.float32(max_h)))
