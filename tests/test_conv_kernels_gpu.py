"""Every convolution kernel family, per element, against the fp64 reference of tests/conv_ref.py -- at the tile, split and pitch edges
where the persistent loops, the rolling halos, the ragged masks and the split hand-offs make more than one trip.

One runner (run_case) serves every row of the tables.  Per placement (dense / the first C channels of a buffer 32 channels wider / the
last C channels) it runs forward, data gradient and both column-sum forms of the weight gradient in poisoned, fenced buffers, and after
each call asserts (1) the kernel family that ran (mi_conv_last_kernel) and the plan's split count against the row, (2) that no fence row
or gap column changed, (3) the comparer: `ints` inputs bit for bit, `gauss` inputs (flagged rows, dense placement) inside the derived
bound.  The rows are derived from the launch code (conv.hip: conv_plan_routes, pick_nsplit, the entry points; conv27.hip / convph.hip
/ conv1x1.hip / conv_c1.hip launch wrappers); a dispatch rule that moves shows as a failed expectation here, not as lost coverage.

Tile 4x8x8 (2-D: 1x16x16), 32-channel chunks.  Shapes are the smallest at which each edge exists:
  tile grid     one tile; one voxel past a tile per axis and on all three (5,9,9); below a tile (3,5,7); tilesH odd / even with tilesD > 1
                (the h-block tile walk switches); two images with ragged tiles; 2-D (1,17,33)
  conv27        <1> plain; rolling from tilesD >= 4 with one 32-channel chunk ((13,9,9) is the smallest); rolling with 450 tiles on
                256 workgroups (a run ends inside a column and the next starts mid-column); <2> from tiles * ceil(C/64) > 128; the
                forced 32-channel rows of 96; ragged last chunk / cout block (40 -> 72); one 8-channel chunk
  table-driven  Cin or Cout not a multiple of 8 (9 -> 32, 4 -> 16, 16 -> 4, 9 -> 256); the 64-channel mode 1 / 2 forms (9 -> 64 and 64 -> 9
                at 2 x 20x32x32); mode 0 with 4 / 6 / 10 / 16 halo pieces per thread (1x1, (1,3,3), strided (2,2,1), k3 s2 at depth 2)
  VGG plans     the (1,3,3) plans of the LPIPS stack: three slices, 8 -> 64 at 8 x 8, 256 -> 512 at 4 x 4, 512 -> 512 at 2 x 2 (one ragged
                tile per slice; 2, 128 and 256 weight-gradient pairs in 3, 2 and 1 splits)
  1x1           streaming with 1, 2, 3, 4, 6 chunks; the NT GEMM (512 -> 256); 32 -> 4 / 4 -> 32 / 4 -> 4 (forward and data gradient on
                different routes); V a multiple of 256 and not; the per-image column sums at V % 256 != 0 (leaves k_wgrad1x1)
  one channel   1 -> C, C -> 1 for C = 8, 64, two images, ragged tiles; the per-image column sums leave k_c1_wgrad for the tiled kernel
  phase         Upsample + conv and k3 s2 both ways; odd fine extents; 1-4 chunks; the 64-channel forms; the residual call that falls back
  weight grad   nsplit 1 with 256 pairs; nsplit == ntiles, contiguous placement (8); 15 ragged splits of 100 tiles; 50 splits (>= 8, not a
                multiple of 8); tilesD == 1 with several tiles (stays on k_conv_wgrad2<true>); s2 in place; upsample pairs;
                register-staged forms (NP 2 / 3 / 5 / 8 and the 3-D one)
The forms behind environment switches run in child processes (the library reads a switch once): SWITCH_SETS.  Two of their rows, the
data gradient of the Upsample FALLBACK (MI_CONVPH=0), are held to conv_ref.folded_dx: that route is two kernels with a bf16 tensor
between them, so it rounds twice by construction (1942 of 16 384 elements differ from the once-rounded sum at 2 x 32 -> 32 (4,8,8), the
same 1942 the two-rounding model predicts); every other row is held to the once-rounded exact result.

Measured on the MI355X: every row passes in all three placements, 0 unequal elements over 1794 comparisons, worst `gauss` ratio 0.99
(bf16 outputs, where the bound's first term is the output rounding itself) and 0.012 (fp32 outputs); slowest row 1.1 s.  EXPERIMENTS.md has
the table per kernel family.
"""
import ctypes as C
import math
import os
import subprocess
import sys
import time

import pytest
import torch

from tests import conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = R.kernel_ids()
NAMES = {v: k[len("MI_CK_"):] for k, v in IDS.items()}
K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
gpu = pytest.mark.gpu


def case(name, n, cin, cout, dims, fwd, dg, wg, splits, k=K3, s=S1, p=P1, up=False, res=False, wg_img=None, sums=False, addrows=False,
         gauss=False, x_dense=False, dx_folded=False):
    """fwd / dg / wg: the kernel family (MI_CK_ name) each direction must run; wg_img: the weight gradient with per-image [N, Cout] column
    sums where that form takes another kernel than the batch form [Cout]; splits: mi_conv_plan_wgrad_splits.  res: forward with a
    residual; sums: the forward also emits GroupNorm sums; addrows: addvec as [N, Cout] rows of a wider matrix; gauss: also run the `gauss`
    kind; x_dense: x stays dense in the pitched placements (the Upsample fallback takes no pitched x); dx_folded: the data gradient runs
    on the Upsample fallback, whose two kernels round twice (conv_ref.folded_dx) -- still bit for bit."""
    for idn in (fwd, dg, wg, wg_img or wg):
        assert "MI_CK_" + idn in IDS, idn
    return dict(name=name, n=n, cin=cin, cout=cout, dims=dims, fwd=fwd, dg=dg, wg=wg, wg_img=wg_img or wg, splits=splits, k=k, s=s, p=p, up=up,
                res=res, sums=sums, addrows=addrows, gauss=gauss, x_dense=x_dense or (up and res), dx_folded=dx_folded)


K1, P0 = (1, 1, 1), (0, 0, 0)
CASES = [
    # ---- tile grid, conv27 <1> plain
    case("one_tile", 1, 32, 32, (4, 8, 8), "C27_1_FWD", "C27_1_DG", "WG2_GEO3", 1),
    case("d5", 1, 32, 32, (5, 8, 8), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 2),
    case("h9", 1, 32, 32, (4, 9, 8), "C27_1_FWD", "C27_1_DG", "WG2_GEO3", 2),
    case("w9", 1, 32, 32, (4, 8, 9), "C27_1_FWD", "C27_1_DG", "WG2_GEO3", 2),
    case("t599", 1, 32, 32, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 8, sums=True),          # nsplit == ntiles == 8: contiguous placement
    case("t357", 1, 32, 32, (3, 5, 7), "C27_1_FWD", "C27_1_DG", "WG2_GEO3", 1),
    case("tilesH3", 1, 32, 32, (5, 17, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 12, sums=True),     # hb = 1
    case("tilesH4", 1, 32, 32, (5, 25, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 16),                # hb = 2
    case("n2_599", 2, 32, 32, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 16, sums=True, addrows=True, res=True),
    case("2d_32to64", 1, 32, 64, (1, 17, 33), "IGEMM_M0_64", "IGEMM_M0_32", "WG2_GEN", 6, k=(1, 3, 3), p=(0, 1, 1), gauss=True),
    case("2d_3to16", 1, 3, 16, (1, 17, 33), "IGEMM_M0_32", "IGEMM_M0_32", "WG_REGS_NP3", 6, k=(1, 3, 3), p=(0, 1, 1), gauss=True),
    case("2d_n2", 2, 32, 64, (1, 16, 16), "IGEMM_M0_64", "IGEMM_M0_32", "WG2_GEN", 2, k=(1, 3, 3), p=(0, 1, 1), res=True, addrows=True),
    # ---- the 2-D plans of the LPIPS VGG stack (perceptual.py: N = slices, (1,3,3) p (0,1,1)), from a 16 x 16 tile's 8 x 8 level down to 2 x 2:
    # one 1 x 16 x 16 tile per slice, so ntiles = 3; pairs = (Cout / 32) x (Cin / 32): 2, 128, 256 -> pick_nsplit gives 3, 2, 1 splits
    case("vgg_8to64", 3, 8, 64, (1, 8, 8), "IGEMM_M0_64", "IGEMM_M0_32", "WG2_GEN", 3, k=(1, 3, 3), p=(0, 1, 1)),
    case("vgg_256to512", 3, 256, 512, (1, 4, 4), "IGEMM_M0_64", "IGEMM_M0_64", "WG2_GEN", 2, k=(1, 3, 3), p=(0, 1, 1)),
    case("vgg_512to512", 3, 512, 512, (1, 2, 2), "IGEMM_M0_64", "IGEMM_M0_64", "WG2_GEN", 1, k=(1, 3, 3), p=(0, 1, 1), gauss=True),
    # ---- conv27 variants
    case("64to64", 1, 64, 64, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 8, gauss=True, res=True),
    case("roll_min", 1, 32, 32, (13, 9, 9), "C27_ROLL_FWD", "C27_ROLL_DG", "WG_ROLL", 16, sums=True, gauss=True, res=True),
    case("roll_trips", 2, 32, 32, (33, 33, 33), "C27_ROLL_FWD", "C27_ROLL_DG", "WG_ROLL", 225, sums=True),   # 450 tiles, grid 256
    case("c27x2_128", 1, 128, 128, (17, 25, 33), "C27_2_FWD", "C27_2_DG", "WG_ROLL", 15),          # 100 ragged tiles in 15 splits
    case("c27x2_64", 1, 64, 64, (17, 33, 41), "C27_2_FWD", "C27_2_DG", "WG_ROLL", 50, gauss=True),  # 150 tiles
    case("32to96", 1, 32, 96, (17, 25, 33), "C27_ROLL_FWD", "C27_1_DG", "WG_ROLL", 50),            # 96: rows of 32 although 100 tiles
    case("96to32", 1, 96, 32, (17, 25, 33), "C27_1_FWD", "C27_ROLL_DG", "WG_ROLL", 50),
    case("40to72", 1, 40, 72, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 8, res=True, sums=True),
    case("8to32", 1, 8, 32, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 8, sums=True),
    case("32to8", 1, 32, 8, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 8),
    case("8to32_d13", 1, 8, 32, (13, 9, 9), "C27_1_FWD", "C27_ROLL_DG", "WG_ROLL", 16),            # rolling needs a whole 32-channel chunk
    case("8to256", 1, 8, 256, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 8),
    case("256to8", 1, 256, 8, (5, 9, 9), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 8),
    # ---- table-driven kernel, register-staged weight gradients
    case("9to32", 1, 9, 32, (5, 9, 9), "IGEMM_M1_32", "IGEMM_M2_32", "WG_REGS_GEO3", 8, gauss=True, res=True),
    case("4to16", 1, 4, 16, (5, 9, 9), "IGEMM_M1_32", "IGEMM_M2_32", "WG_REGS_GEO3", 8),
    case("16to4", 1, 16, 4, (5, 9, 9), "IGEMM_M1_32", "IGEMM_M2_32", "WG_REGS_GEO3", 8),
    case("9to64", 2, 9, 64, (20, 32, 32), "IGEMM_M1_64", "IGEMM_M2_32", "WG_REGS_GEO3", 80, gauss=True, res=True),
    case("64to9", 2, 64, 9, (20, 32, 32), "IGEMM_M1_32", "IGEMM_M2_64", "WG_REGS_GEO3", 80, gauss=True),
    case("9to256", 1, 9, 256, (5, 9, 9), "IGEMM_M1_32", "IGEMM_M2_32", "WG_REGS_GEO3", 8),
    case("s221", 1, 32, 32, (8, 8, 4), "IGEMM_M0_32", "IGEMM_M0_32", "WG2_GEN", 1, k=(3, 3, 1), s=(2, 2, 1), p=(1, 1, 0), gauss=True),
    case("s221_8to12", 1, 8, 12, (9, 10, 5), "IGEMM_M0_32", "IGEMM_M0_32", "WG_REGS_NP5", 2, k=(3, 3, 1), s=(2, 2, 1), p=(1, 1, 0), gauss=True),
    case("2d_s122", 1, 64, 64, (1, 20, 12), "IGEMM_M0_64", "IGEMM_M0_64", "WG2_GEN", 1, k=(1, 3, 3), s=(1, 2, 2), p=(0, 1, 1)),
    case("s2_d2", 1, 32, 32, (2, 16, 16), "IGEMM_M0_32", "IGEMM_M0_32", "WG_REGS_NP8", 1, s=(2, 2, 2), gauss=True),   # depth 2: no phase kernels, 16 pieces
    # ---- 1x1
    case("1x1_32", 1, 32, 32, (4, 8, 8), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 1, k=K1, p=P0),
    case("1x1_64", 1, 64, 64, (4, 8, 9), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 2, k=K1, p=P0, wg_img="WG2_GEN_1X1", gauss=True),
    case("1x1_96", 1, 96, 96, (4, 8, 8), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 1, k=K1, p=P0),
    case("1x1_128", 1, 128, 128, (4, 8, 9), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 2, k=K1, p=P0, wg_img="WG2_GEN_1X1"),
    case("1x1_192", 1, 192, 192, (4, 8, 8), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 1, k=K1, p=P0),
    case("1x1_gemm", 1, 512, 256, (4, 8, 8), "1X1_GEMM", "1X1_GEMM", "WG_1X1", 1, k=K1, p=P0, gauss=True),
    case("1x1_gemm_rag", 2, 384, 128, (3, 5, 7), "1X1_GEMM", "1X1_STREAM", "WG_1X1", 2, k=K1, p=P0, wg_img="WG2_GEN_1X1"),
    case("1x1_32to4", 1, 32, 4, (4, 8, 9), "1X1_STREAM", "IGEMM_M0_32", "WG_REGS_NP2", 2, k=K1, p=P0),
    case("1x1_4to4", 1, 4, 4, (4, 8, 9), "IGEMM_M0_32", "IGEMM_M0_32", "WG_REGS_NP2", 2, k=K1, p=P0, gauss=True),
    case("1x1_4to32", 1, 4, 32, (4, 8, 9), "IGEMM_M0_32", "1X1_STREAM", "WG_REGS_NP2", 2, k=K1, p=P0),
    case("1x1_n2_rag", 2, 64, 32, (4, 8, 9), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 4, k=K1, p=P0, wg_img="WG2_GEN_1X1", addrows=True),
    case("1x1_n2_256", 2, 64, 32, (4, 8, 8), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 2, k=K1, p=P0),
    case("1x1_2d", 2, 8, 8, (1, 5, 7), "1X1_STREAM", "1X1_STREAM", "WG_1X1", 2, k=K1, p=P0, wg_img="WG2_GEN_1X1"),
    # ---- one channel on one side
    case("c1_1to8", 2, 1, 8, (5, 9, 11), "C1_EXPAND", "IGEMM_M2_32", "WG_C1", 16, wg_img="WG_REGS_GEO3", sums=True, addrows=True, gauss=True),
    case("c1_1to64", 2, 1, 64, (5, 9, 11), "C1_EXPAND", "IGEMM_M2_32", "WG_C1", 16, wg_img="WG_REGS_GEO3"),
    case("c1_8to1", 2, 8, 1, (5, 9, 11), "C1_REDUCE", "C1_EXPAND", "WG_C1", 16, wg_img="WG_REGS_GEO3", gauss=True),
    case("c1_64to1", 2, 64, 1, (5, 9, 11), "C1_REDUCE", "C1_EXPAND", "WG_C1", 16, wg_img="WG_REGS_GEO3"),
    # ---- phase kernels
    case("up_32", 2, 32, 32, (4, 8, 8), "PH_SCATTER_32", "PH_GATHER_32", "WG_UP", 2, up=True, addrows=True),
    case("up_64_odd", 1, 64, 64, (5, 9, 11), "PH_SCATTER_32", "PH_GATHER_32", "WG_UP", 8, up=True),
    case("up_96", 1, 96, 64, (3, 5, 7), "PH_SCATTER_32", "PH_GATHER_32", "WG_UP", 1, up=True),
    case("up_128", 1, 128, 32, (4, 8, 8), "PH_SCATTER_32", "PH_GATHER_32", "WG_UP", 1, up=True),
    case("up_8to128", 1, 8, 128, (17, 17, 33), "PH_SCATTER_64", "PH_GATHER_32", "WG_UP", 25, up=True),     # 75 coarse tiles x 2 blocks of 64
    case("up_res", 1, 32, 32, (4, 8, 8), "C27_1_FWD", "PH_GATHER_32", "WG_UP", 1, up=True, res=True),      # a residual: the fallback's inner plan
    case("s2_32", 1, 32, 32, (8, 8, 8), "PH_GATHER_32", "PH_SCATTER_32", "WG2_GEN_DIRECT", 1, s=(2, 2, 2)),
    case("s2_odd", 2, 96, 64, (7, 9, 11), "PH_GATHER_32", "PH_SCATTER_32", "WG2_GEN_DIRECT", 2, s=(2, 2, 2), gauss=True),
    case("s2_8to128", 1, 8, 128, (33, 33, 65), "PH_GATHER_64", "PH_SCATTER_32", "WG2_GEN", 8, s=(2, 2, 2), gauss=True),  # Cin % 32 != 0: space-to-depth x
    case("s2_128", 1, 128, 128, (16, 16, 16), "PH_GATHER_32", "PH_SCATTER_32", "WG2_GEN_DIRECT", 2, s=(2, 2, 2)),
    # ---- weight-gradient splits
    case("512to512", 1, 512, 512, (4, 8, 8), "C27_1_FWD", "C27_1_DG", "WG2_GEO3", 1, gauss=True),   # one split, 256 pairs
    case("tilesD1_multi", 1, 32, 32, (4, 17, 17), "C27_1_FWD", "C27_1_DG", "WG2_GEO3", 9),         # 9 tiles, tilesD == 1: not rolling
]
BY_NAME = {c["name"]: c for c in CASES}
# split forms the tables must contain: name -> (case, what it is)
SPLIT_FORMS = {"one split, many pairs": "512to512", "nsplit == ntiles, contiguous": "t599", "ragged, several tiles per workgroup": "c27x2_128",
               ">= 8 and not a multiple of 8": "c27x2_64", "tilesD == 1, several tiles": "tilesD1_multi", "s2 in place": "s2_32",
               "upsample pairs": "up_64_odd", "register-staged": "9to32"}
# ids no default-switch dispatch reaches: none.  (Every family has a row above.)
SWITCH_ONLY = set()

# the weights of these go through mi_conv_pack_batch_* (what the trainers run every step) instead of mi_conv_pack_weights
BATCH_PACK = ["t599", "40to72", "9to32", "s2_odd", "up_64_odd", "1x1_gemm", "c1_1to8", "c1_8to1"]


def _with(name, **kw):
    return dict(BY_NAME[name], **kw)


# environment switches -> the rows that run under them in ONE child process (kernel ids as the dispatch gives them with the switch set)
SWITCH_SETS = {
    "conv27_off": (dict(MI_CONV27="0"), [
        _with("t599", fwd="IGEMM_M1_32", dg="IGEMM_M2_32", sums=False), _with("64to64", fwd="IGEMM_M1_32", dg="IGEMM_M2_32", gauss=False),
        _with("c27x2_64", fwd="IGEMM_M1_64", dg="IGEMM_M2_64", gauss=False)]),
    "wgrad2_off": (dict(MI_WGRAD2="0"), [
        _with("t599", wg="WG_REGS_GEO3", wg_img="WG_REGS_GEO3"), _with("2d_32to64", wg="WG_REGS_NP3", wg_img="WG_REGS_NP3", gauss=False),
        _with("s2_32", wg="WG_REGS_NP5", wg_img="WG_REGS_NP5")]),
    "roll_off": (dict(MI_C27_ROLL="0", MI_WGRAD_ROLL="0"), [
        _with("roll_min", fwd="C27_1_FWD", dg="C27_1_DG", wg="WG2_GEO3", wg_img="WG2_GEO3", gauss=False),
        _with("n2_599", wg="WG2_GEO3", wg_img="WG2_GEO3")]),
    "conv1x1_off": (dict(MI_CONV1X1="0", MI_CONV1X1_GEMM="0", MI_WGRAD1X1="0"), [
        _with("1x1_64", fwd="IGEMM_M0_32", dg="IGEMM_M0_32", wg="WG2_GEN_1X1", wg_img="WG2_GEN_1X1", gauss=False),
        _with("1x1_gemm", fwd="IGEMM_M0_32", dg="IGEMM_M0_32", wg="WG2_GEN_1X1", wg_img="WG2_GEN_1X1", gauss=False),
        _with("1x1_n2_256", fwd="IGEMM_M0_32", dg="IGEMM_M0_32", wg="WG2_GEN_1X1", wg_img="WG2_GEN_1X1")]),
    "c1_off": (dict(MI_CONV_C1="0", MI_C1_WGRAD="0"), [
        _with("c1_1to8", fwd="IGEMM_M1_32", dg="IGEMM_M2_32", wg="WG_REGS_GEO3", wg_img="WG_REGS_GEO3", sums=False, gauss=False),
        _with("c1_8to1", fwd="IGEMM_M1_32", dg="IGEMM_M2_32", wg="WG_REGS_GEO3", wg_img="WG_REGS_GEO3", gauss=False)]),
    "cs_slab_off": (dict(MI_CS_SLAB="0"), [_with("n2_599"), _with("2d_32to64", gauss=False), _with("s2_odd", gauss=False)]),
    "pack_super_off": (dict(MI_PACK_SUPER="0"), [_with(n, gauss=False, batch_pack=True) for n in ("t599", "40to72", "s2_odd", "1x1_gemm")]),
    # the routes behind the phase kernels (the cases of test_conv_routes_gpu.py, which keeps its own assertions): the Upsample fallback
    # (inner k3 s1 plan on the fine grid; x must be dense) and the space-to-depth forms of an all-axes k3 s2 conv
    "convph_off": (dict(MI_CONVPH="0"), [
        _with("up_32", fwd="C27_1_FWD", dg="C27_1_DG", wg="WG_ROLL", wg_img="WG_ROLL", splits=16, x_dense=True, dx_folded=True),
        case("up_64to32", 2, 64, 32, (3, 5, 7), "C27_1_FWD", "C27_1_DG", "WG_ROLL", 16, up=True, x_dense=True, dx_folded=True),
        _with("s2_32", fwd="IGEMM_M0_32", dg="IGEMM_M0_32", wg="WG2_GEN", wg_img="WG2_GEN"),
        case("s2_64", 1, 64, 64, (6, 10, 12), "IGEMM_M0_32", "IGEMM_M0_32", "WG2_GEN", 1, s=(2, 2, 2))]),
}


def test_cases_reach_every_kernel_family():
    """Needs no GPU: the union of the expected ids of the default-switch tables covers the whole enum, and every split form has its row."""
    reached = set()
    for c in CASES:
        reached.update((c["fwd"], c["dg"], c["wg"], c["wg_img"]))
    every = {n for n in NAMES.values() if n not in ("NONE", "COUNT")}
    assert every - reached - SWITCH_ONLY == set(), sorted(every - reached - SWITCH_ONLY)
    for what, name in SPLIT_FORMS.items():
        assert name in BY_NAME, what
    c = BY_NAME
    assert c["512to512"]["splits"] == 1 and c["t599"]["splits"] == 8 and c["c27x2_128"]["splits"] == 15 and c["c27x2_64"]["splits"] == 50
    assert c["c27x2_64"]["splits"] >= 8 and c["c27x2_64"]["splits"] % 8 != 0
    assert c["tilesD1_multi"]["wg"] == "WG2_GEO3" and c["tilesD1_multi"]["splits"] > 1
    assert c["s2_32"]["wg"] == "WG2_GEN_DIRECT" and c["up_64_odd"]["wg"] == "WG_UP" and c["9to32"]["wg"] == "WG_REGS_GEO3"
    assert {c[n]["wg"] for n in ("1x1_4to4", "2d_3to16", "s221_8to12", "s2_d2")} == {"WG_REGS_NP2", "WG_REGS_NP3", "WG_REGS_NP5", "WG_REGS_NP8"}
    for env, rows in SWITCH_SETS.values():
        assert 2 <= len(rows) <= 4 and all(k.startswith("MI_") for k in env)


# ----------------------------------------------------------------------------------------------------------------- the runner
def out_dims_of(c):
    if c["up"]:
        return tuple(2 * d for d in c["dims"])
    return tuple((d + 2 * p - k) // s + 1 for d, k, s, p in zip(c["dims"], c["k"], c["s"], c["p"]))


def _last(ops):
    return NAMES.get(ops.ConvPlan.last_kernel(), "?")


def _pack(ops, plan, w, batch):
    if not batch:
        plan.pack(w)
        return
    from medical_image_generation_amd import _lib
    h = C.c_void_p()
    _lib.call_raw("mi_conv_pack_batch_create", C.byref(h), (C.c_void_p * 1)(plan.handle), (C.c_void_p * 1)(w.data_ptr()), 1)
    try:
        _lib.call("mi_conv_pack_batch_run", h)
        torch.cuda.synchronize()
    finally:
        _lib.call_raw("mi_conv_pack_batch_destroy", h)


def run_case(ops, c, kind, placements, report=print):
    """Every direction of one row in the given placements; returns [(placement, quantity, kernel, worst)] and raises on the first miss."""
    from medical_image_generation_amd import _lib
    dev = torch.device("cuda")
    n, cin, cout, dims, k, s, p, up = (c[q] for q in ("n", "cin", "cout", "dims", "k", "s", "p", "up"))
    od = out_dims_of(c)
    if kind == "ints":
        R.check_exact_range(n, cin, cout, od, k, up)
    t = R.make_inputs(kind, n, cin, cout, dims, k, od, up=up)
    ref = R.reference(t, s, p, up, "rows" if c["addrows"] else "bias", with_abs=(kind == "gauss"))
    nt = R.terms(n, cin, cout, od, k, up)
    res64 = t["res"] if c["res"] else None
    bnd = R.gauss_bounds(ref, nt, res64) if kind == "gauss" else None
    y_want = R.cl(R.expected_y(ref, res64, kind))
    plan = ops.UpConvPlan(n, dims, cin, cout) if up else ops.ConvPlan(n, dims, cin, cout, k, s, p)
    assert plan.out_dims == od
    assert plan.wgrad_splits == c["splits"], f"{c['name']}: {plan.wgrad_splits} weight-gradient splits, the table says {c['splits']}"
    w32 = t["w"].to(torch.float32).to(dev)
    _pack(ops, plan, w32, c.get("batch_pack", False))
    if c["addrows"]:
        wide = torch.full((n, cout + 8), math.nan, dtype=torch.float32)
        wide[:, 4:4 + cout] = t["addrows"].float()
        addvec = wide.to(dev)[:, 4:4 + cout]
    else:
        addvec = t["bias"].float().to(dev)
    xsh, ysh = (n,) + tuple(dims) + (cin,), (n,) + od + (cout,)
    rows = []

    def check(pl, q, want_id, slot, ref2d, bound2d=None):
        got_id = _last(ops)
        assert got_id == want_id, f"{c['name']} [{pl}] {q}: ran {got_id}, the table says {want_id}"
        worst, fences = R.compare(kind, slot, ref2d, bound2d)
        report(f"CONVCASE {c['name']} {kind} {pl} {q} {got_id} {worst:.6g} fences={'ok' if fences else 'BROKEN'}")
        rows.append((pl, q, got_id, worst))
        assert fences, f"{c['name']} [{pl}] {q} ({got_id}): a fence row or gap column changed"
        if kind == "ints":
            assert worst == 0, f"{c['name']} [{pl}] {q} ({got_id}): {worst} elements differ from the exact result"
        else:
            assert worst <= 1.0, f"{c['name']} [{pl}] {q} ({got_id}): err / bound = {worst}"

    for pl in placements:
        plx = "dense" if c["x_dense"] else pl
        xs = R.Slot(xsh, plx, R.cl(t["x"]), dev)
        dys = R.Slot(ysh, pl, R.cl(t["dy"]), dev)
        rs = R.Slot(ysh, pl, R.cl(t["res"]), dev) if c["res"] else None
        # ---- forward
        ys = R.Slot(ysh, pl, device=dev)
        plan.fwd(xs.view(), addvec=addvec, res=rs.view() if rs else None, out=ys.view())
        check(pl, "y", c["fwd"], ys, y_want, R.cl(bnd["y"]) if bnd else None)
        if c["sums"] and kind == "ints":
            ys2 = R.Slot(ysh, pl, device=dev)
            _, sums = plan.fwd(xs.view(), addvec=addvec, res=rs.view() if rs else None, out=ys2.view(), want_sums=True)
            assert sums is not None, f"{c['name']} [{pl}]: the forward emitted no GroupNorm sums"
            assert _last(ops) == c["fwd"] and ys2.fences_intact()
            assert torch.equal(ys2.payload().view(torch.int16), ys.payload().view(torch.int16)), f"{c['name']} [{pl}]: y differs with sums"
            y = ys.payload().double().cpu().view(n, -1, cout)
            part = sums.partial.double().cpu().sum(dim=2)                   # [n, cout, 2]
            unit = R.SCALE["x"] * R.SCALE["w"]                              # every y is a whole number of these
            assert float(y.abs().sum(dim=1).max()) / unit < 2 ** 24, "the sum of y is not exact in fp32 at this shape"
            assert torch.equal(part[..., 0], y.sum(dim=1)), f"{c['name']} [{pl}]: sum of y {float((part[..., 0] - y.sum(dim=1)).abs().max())} off"
            ssq = (y * y).sum(dim=1)
            lim = y.shape[1] * R.U23 * ssq
            assert bool(((part[..., 1] - ssq).abs() <= lim).all()), f"{c['name']} [{pl}]: sum of y^2 outside V 2^-23 sum(y^2)"
        # ---- data gradient (dx dense, as hipops allocates it, but fenced: through the C ABI)
        dxs = R.Slot(xsh, "dense", device=dev)
        _lib.call("mi_conv_dgrad", plan.handle, dys.view().data_ptr(), dys.width, dxs.view().data_ptr(), cin)
        check(pl, "dx", c["dg"], dxs, R.cl(R.folded_dx(ref) if c["dx_folded"] else ref["dx"]), R.cl(bnd["dx"]) if bnd else None)
        # ---- weight gradient into a non-zero prefill, both column-sum forms
        for form, want_id in (("img", c["wg_img"]), ("batch", c["wg"])):
            dws = R.SlotF32(t["dw0"].reshape(1, -1), device=dev)
            css = R.SlotF32(t["cs0_img"], pitched=(pl != "dense"), device=dev) if form == "img" else R.SlotF32(t["cs0"][None], device=dev)
            plan.wgrad(xs.view(), dys.view(), dws.view().view(t["w"].shape), colsum=css.view() if form == "img" else css.view()[0])
            dw_want = ref["dw"] + t["dw0"]
            cs_want = ref["cs_img"] + t["cs0_img"] if form == "img" else (ref["cs"] + t["cs0"])[None]
            if bnd:
                bdw = nt["dw"] * R.U23 * (ref["A_dw"] + t["dw0"].abs())
                bcs = (nt["cs_img"] * R.U23 * (ref["A_cs_img"] + t["cs0_img"].abs())) if form == "img" else (nt["cs"] * R.U23 * (ref["A_cs"] + t["cs0"].abs())[None])
            check(pl, "dw_" + form, want_id, dws, dw_want, bdw if bnd else None)
            check(pl, "cs_" + form, want_id, css, cs_want, bcs if bnd else None)
    torch.cuda.synchronize()
    return rows


@pytest.fixture(scope="module")
def ops():
    from medical_image_generation_amd import hipops
    return hipops


@gpu
def test_mfma_accumulates_integers_exactly(ops):
    """The premise of the `ints` contract: where the exact sum fits 24 bits the fp32 MFMA accumulator holds it, whatever the order.  Integer
    bf16 matrices with K = 27 * 512 through the NT GEMM against an int64 matmul, bit for bit."""
    g = torch.Generator().manual_seed(5)
    m, n, k = 96, 160, 27 * 512
    a = torch.randint(-4, 5, (m, k), generator=g)
    b = torch.randint(-4, 5, (n, k), generator=g)
    want = a @ b.T
    assert int((a.abs() @ b.abs().T).max()) < 2 ** 24
    got = ops.gemm_nt(a.to(torch.bfloat16).cuda(), b.to(torch.bfloat16).cuda(), out_f32=True).cpu()
    assert got.dtype == torch.float32 and torch.equal(got.to(torch.int64), want) and torch.equal(got, want.float())


@gpu
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_conv_case(ops, name):
    c = BY_NAME[name]
    t0 = time.time()
    run_case(ops, c, "ints", R.PLACEMENTS)
    if c["gauss"]:
        run_case(ops, c, "gauss", ("dense",))
    print(f"CONVTIME {name} {time.time() - t0:.2f} s")


@gpu
@pytest.mark.parametrize("name", BATCH_PACK)
def test_conv_case_batch_pack(ops, name):
    """The same rows with the weights packed by mi_conv_pack_batch_run, the pack the trainers run every step."""
    run_case(ops, dict(BY_NAME[name], batch_pack=True, sums=False), "ints", ("dense", "last"))


@gpu
def test_rolling_weight_gradient_repeats_bit_for_bit(ops):
    """k_conv_wgrad3 at 1 x 64^3, 128 -> 64: 1024 tiles in 32 splits, four cin chunks -- many tiles per workgroup under load.  With `ints`
    inputs the sums are exact, so every run of one plan must equal the first bit for bit.  With one running hand-off count per direction
    (instead of one per parity of the tile number) a wave that was a tile ahead could stand in for a lagging one, and 1 to 6 of 59
    repeats came back with one 32 x 32 block of a tap wrong; the exact result itself is pinned by the `roll_trips` / `c27x2_*` rows."""
    n, cin, cout, dims = 1, 128, 64, (64, 64, 64)
    R.check_exact_range(n, cin, cout, dims, K3)
    t = R.make_inputs("ints", n, cin, cout, dims, K3, dims)
    plan = ops.ConvPlan(n, dims, cin, cout, K3, S1, P1)
    assert plan.wgrad_splits == 32
    plan.pack(t["w"].float().cuda())
    xs = R.Slot((n,) + dims + (cin,), "dense", R.cl(t["x"]), "cuda")
    dys = R.Slot((n,) + dims + (cout,), "dense", R.cl(t["dy"]), "cuda")
    first, differ = None, 0
    for _ in range(60):
        dw = torch.zeros(t["w"].shape, dtype=torch.float32, device="cuda")
        plan.wgrad(xs.view(), dys.view(), dw)
        assert _last(ops) == "WG_ROLL"
        if first is None:
            first = dw
        else:
            differ += int(not torch.equal(dw, first))
    assert differ == 0, f"{differ} of 59 repeats differ from the first"


def child_main(set_name):
    """Body of a switch child: the environment is already set by the parent."""
    from medical_image_generation_amd import hipops
    for c in SWITCH_SETS[set_name][1]:
        run_case(hipops, c, "ints", R.PLACEMENTS)
    torch.cuda.synchronize()
    print("SWITCH SET OK " + set_name)


@gpu
@pytest.mark.parametrize("set_name", list(SWITCH_SETS))
def test_forms_behind_switches(set_name):
    """What production falls to when a pitch or a channel count disqualifies the fast route, held to the same contract: a fresh child
    process per switch set (the library reads a switch once), one at a time, each under its own time limit."""
    env = dict(os.environ, **SWITCH_SETS[set_name][0])
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_conv_kernels_gpu import child_main; child_main({set_name!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    sys.stdout.write(r.stdout[-6000:])
    assert r.returncode == 0 and ("SWITCH SET OK " + set_name) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
