"""Builds and loads tests/hostsim/libblur_masks_host.so (TEST HARNESS ONLY): the blur chain on the host with the replayed
iterations through blur_replay_tile or through the split body (csrc/blur_tiles.hpp blur_replay_tile_split), and the frames the
tests of the paired chain kernel share (tests/test_blur_replay_masks_host.py, tests/test_blur_chain_pairs_gpu.py)."""
import ctypes as C
import os

import numpy as np

import hostsim_lib

SRC = os.path.join(hostsim_lib.ROOT, "tests", "hostsim", "blur_masks.cpp")
LIB = os.path.join(hostsim_lib.ROOT, "tests", "hostsim", "libblur_masks_host.so")
STAMP = 1


def build():
    return hostsim_lib.build_host(LIB, SRC, ("ssao_core.hpp", "blur_tiles.hpp"))


def tiles_x(W):
    return (W // 2 + 63) // 64


def tiles_y(H):
    return (H // 2 + 15) // 16


class BlurMasksHost:
    def __init__(self):
        self.lib = C.CDLL(build())
        vp, u32, i = C.c_void_p, C.c_uint32, C.c_int
        self.lib.bm_blur_chain.argtypes = [vp, vp, vp, vp, u32, u32, i, u32, u32, u32, i, i, u32, vp]

    def compute_ssao(self, hostsim, cb, normal, depth, randvec, edge_bytes, blur_count, body, row0=0, rows=None, poison=0):
        """Ssao::ComputeSsao as api.cpp sequences it: hostsim's SSAO pass (stamp STAMP), then bm_blur_chain with the replayed
        iterations through `body` (0: blur_replay_tile, 1: the split body).  Returns (ambient0, settled): rows [row0, row0 + rows)
        of ambient0 are the result; settled[ty, tx] = 1 where the pair launch settled the tile (blur_count > 1)."""
        H, W = depth.shape
        h2 = H // 2
        rows = h2 - row0 if rows is None else rows
        r0, rn = C.c_uint32(), C.c_uint32()
        hostsim.lib.hs_blur_chain_ssao_rows(blur_count, row0, rows, h2, C.addressof(r0), C.addressof(rn))
        out, edge = hostsim.ssao(cb, normal, depth, randvec, edge_bytes, r0.value, rn.value, stamp=STAMP)
        planes = [np.full((h2, W // 2), 0xABCD, dtype=np.uint16), np.full((h2, W // 2), 0xABCD, dtype=np.uint16)]     # junk where nothing writes
        sp = hostsim.lib.hs_blur_chain_ssao_plane(blur_count)
        planes[sp][r0.value:r0.value + rn.value] = out[r0.value:r0.value + rn.value]
        settled = np.zeros((tiles_y(H), tiles_x(W)), np.uint8)
        self.lib.bm_blur_chain(C.addressof(cb), edge.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data, W, H, blur_count, row0, rows,
                               STAMP, 5 * blur_count, body, poison, settled.ctypes.data)
        return planes[0], settled


_BM = None


def load():
    global _BM
    if _BM is None:
        _BM = BlurMasksHost()
    return _BM


# ---- the frames ------------------------------------------------------------------------------------------------------------------
# fuzz_util.rough_wall_case (no tile settles, every texel changes under the blur, so one stale or misplaced word shows), with
# rectangles of sky (full-res x0, y0, x1, y1) laid over it where a case wants tiles to settle.
# name: (W, H, sky rectangles).  Tile columns / rows of the half-res 64 x 16 grid:
#   322 x 190   3 x 6: the last workgroup of a row has a lone tile, whose right edge is ragged (161 = 2 * 64 + 33 columns)
#   128 x 64    1 x 2: every workgroup has one tile and no partner
#   260 x 70    3 x 3 (130 columns: the lone tile is 2 columns wide; 35 rows: the last tile row has 3)
#   512 x 416   4 x 13: two full pairs per tile row
#   sky         512 x 416 with sky that settles the left tile only of pair 0 (top), the right tile only of pair 1 (middle) and
#               whole tile rows (bottom).  A tile settles when the unoccluded-wavefront map, whose cells are 64 columns wide,
#               is all ones on the tile's own cell column and both neighbouring ones, so the top rectangle ends inside cell
#               column 2 and the middle one begins inside cell column 1; the counts are checked with the pair launch's own
#               predicate (pair_cases)
FRAMES = {
    "322x190": (322, 190, ()),
    "128x64": (128, 64, ()),
    "260x70": (260, 70, ()),
    "512x416": (512, 416, ()),
    "sky": (512, 416, ((0, 0, 280, 150), (232, 160, 512, 290), (0, 300, 512, 416))),
}


def frame(name, seed=3):
    """-> (W, H, c, scb, depth, normal, randvec) of FRAMES[name]."""
    import fuzz_util
    W, H, sky = FRAMES[name]
    c, scb, depth, normal, randvec = fuzz_util.rough_wall_case(seed, W, H, False)
    for x0, y0, x1, y1 in sky:
        depth[y0:y1, x0:x1] = 0xFFFFFF
        normal[y0:y1, x0:x1, :3] = (0, 0, -1)
    return W, H, c, scb, depth, normal, randvec


def pair_cases(settled):
    """How the chain kernel's workgroups (two horizontally adjacent tiles each) find their pairs: counts of (left only settled,
    right only settled, both, neither) over the pairs that have both tiles."""
    l, r = settled[:, 0::2][:, :settled.shape[1] // 2] != 0, settled[:, 1::2] != 0
    return int((l & ~r).sum()), int((~l & r).sum()), int((l & r).sum()), int((~l & ~r).sum())
