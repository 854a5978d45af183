"""One row per bf16-split GEMM build: the cases tests/test_split_arithmetic_gpu.py measures against float64 on both matrix paths, and
tests/test_split_cases_cpu.py keeps complete (every kernel family with a split build has a row or a stated exemption) and well formed
(every conv shape passes conv_geo's checks, gather_gemm.hip).  Plain data, no pytest.

A row names the ABI entry it calls, the shape, the epilogue arguments, the patch / wgrad-tile mode where it needs a non-default one,
the axis its cancellation family pairs terms along, and the EXACT kernel timer names (convnet_hip_profile_report) that must appear
when it runs on the split path: a silent change in dispatch fails the row instead of leaving it vacuous.

Conv shapes are (N, C, H, W, F, Ky, Kx, sy, sx, pad) with pad >= 0; FC shapes are (N, D, F): in (N, D), W (F, D), out (N, F);
local shapes as conv with the bank (M, C, Ky, Kx, F)."""
from dataclasses import dataclass


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                  # convUp convUpBiasAct convDown convDownMask convOutpGemm convOutpBias dot dotBiasAct dotMask localUp ...
    shape: tuple
    expect: tuple               # timer names that must all appear on the split path
    st: float = 0.0             # scaleTargets (dot: beta)
    so: float = 1.0             # scaleOutput (dot: alpha)
    relu: int = 0
    post_scale: float = 1.0
    trans: str = ""             # dot: "NT" (out = in W^T), "NN" (din = dout W), "TN" (dW = dout^T in)
    patch_mode: int = -1        # convnet_hip_set_patch_mode for the call (-1: the library default)
    wgrad_tile: int = -1        # convnet_hip_set_wgrad_tile for the call (-1: the library default)
    axis: str = ""              # what the cancellation family pairs: channels / taps / filters / images / d / f / n
    fp32: bool = False          # a launch that runs the fp32 instruction even on the split path (pinned: expect has no ",split")
    note: str = ""
    bounds: tuple = ()          # ((family, (ratio, floor, cap)), ...): a row-specific bound, see ROW_BOUNDS

    def bound(self, kind):
        """the row's (ratio, floor, cap) for a data family, or None for the shared BOUNDS of tests/test_split_arithmetic_gpu.py"""
        return dict(self.bounds).get(kind)

    @property
    def op(self):
        return {"convUp": "fprop", "convUpBiasAct": "fprop", "convDown": "dgrad", "convDownMask": "dgrad", "convOutpGemm": "wgrad",
                "convOutpBias": "wgrad", "localUp": "local_up", "localUpBiasAct": "local_up", "localDown": "local_down",
                "localOutp": "local_outp"}.get(self.entry) or {"NT": "fc_nt", "NN": "fc_nn", "TN": "fc_tn"}[self.trans]

    @property
    def direction(self):
        """forward / input gradient (all five data families) or weight gradient (no 'huge': the sums overflow on any path)"""
        return "wgrad" if self.op in ("wgrad", "fc_tn", "local_outp") else "fwd"


# Row-specific bounds, each set from the value measured on the MI355X (profiles/split_error_builds.txt) with the margin stated; the shared
# BOUNDS are untouched.  Every one is a property documented in include/convnet_hip.h (convnet_hip_set_matrix_path), not a kernel defect:
#  * TINY: |x| ~ 2^-116 operands lose their denormal second / third split terms (the matrix pipe flushes bf16 denormals).  Over the
#    outputs these rows sample (every output of the FC and local rows) the loss reaches 55.8 units (2^-18.2) at 12.2 x the fp32 path;
#    bound 2 x both.
#  * cancellation caps (_cancel_cap): pairs that cancel along taps (C = 3) or on the shorter reductions leave partial sums that both
#    paths round; the fp32 path itself measures up to 0.37 units on the conv rows (0.96 on the local rows) (fallback_gg_nonvector: the same kernel on both paths)
#    and the split path stays within 2 x of it.  Cap ~2 x the split path's measured value.  In emulation (tests/emu/prec.h) a split
#    build without its m*m product measures 3.7-42 units on cancelling data and 6-38 on N(0,1) data, a zero l plane 25-74 on N(0,1)
#    data: every cap here still fails both.
#  * the normal / huge ratio of a few rows: the two paths run different launches (k order, split-K / tail plan, tile) whose maxima
#    over the sampled outputs differ by up to 1.3 x (2-2.4 x where path 0 splits the reduction and path 1 does not); both well below
#    the shared absolute cap.  Measured ratio x 1.5.
TINY = (24.0, 0.0, 112.0)
_TINY = (('tiny', TINY),)   # only on the rows that miss the shared tiny bound


def _cancel_cap(cap):
    return (("cancellation", (16.0, 0.0, cap)),)


GG2 = "ggp_kernel<2,2,2,128,split,pre>"
GG3 = "ggp_kernel<1,4,3,64,split,pre>"
GG1 = "ggp_kernel<2,2,1,128,split,pre>"
GPW = "gpw_kernel<128x512,split,raw>"

CASES = [
    # ---- forward convolution ------------------------------------------------------------------------------------------------------
    Case("fwd_gfc", "convUp", (64, 3, 32, 32, 96, 7, 7, 2, 2, 2), ("gfc_kernel<96x128,split>",), axis="taps", note="conv1 type", bounds=_cancel_cap(0.8)),
    Case("fwd_gfc_accumulate", "convUp", (64, 3, 32, 32, 96, 7, 7, 2, 2, 2), (GG3,), st=0.75, axis="taps",
         note="gfc_kernel refuses scaleTargets != 0: the generic-k producer kernel takes it", bounds=_cancel_cap(0.9) + (('normal', (2.0, 1.0, 8.0)),)),
    Case("fwd_gfc_bias_relu", "convUpBiasAct", (64, 3, 32, 32, 96, 7, 7, 2, 2, 2), ("gfc_kernel<96x128,split>",), relu=1, axis="taps", bounds=(('huge', (2.0, 1.0, 8.0)),) + _cancel_cap(0.8)),
    Case("fwd_generic_k", "convUp", (48, 3, 24, 24, 96, 7, 7, 2, 2, 2), (GG3,), axis="taps", note="N % 32 != 0: gfc_kernel refuses", bounds=_cancel_cap(1.4)),
    Case("fwd_generic_k_c88", "convUp", (32, 88, 12, 12, 128, 3, 3, 1, 1, 1), (GG2,), axis="channels", note="C % 16 != 0, F > 96, K = 792", bounds=_TINY + _cancel_cap(0.7)),
    Case("fwd_ggp_r128", "convUp", (32, 128, 9, 9, 128, 3, 3, 1, 1, 1), (GG2,), axis="channels", bounds=_TINY),
    Case("fwd_ggp_r96", "convUp", (32, 128, 9, 9, 80, 3, 3, 1, 1, 1), (GG3,), axis="channels", bounds=_TINY),
    Case("fwd_ggp_r64", "convUp", (32, 128, 9, 9, 48, 3, 3, 1, 1, 1), (GG1,), axis="channels", bounds=_TINY),
    Case("fwd_ggp_bias_relu", "convUpBiasAct", (32, 128, 9, 9, 128, 3, 3, 1, 1, 1), (GG2,), relu=1, axis="channels", bounds=_TINY),
    Case("fwd_ggp_splitk", "convUp", (32, 256, 6, 6, 128, 3, 3, 1, 1, 1), (GG2, "gg_reduce_kernel"), axis="channels",
         note="5 tiles, 144 k-chunks: split-K and the slab reduce", bounds=_TINY),
    Case("fwd_ggp_splitk_accumulate", "convUpBiasAct", (32, 256, 6, 6, 128, 3, 3, 1, 1, 1), (GG2, "gg_reduce_kernel"), st=0.5, relu=1,
         axis="channels", note="scaleTargets, bias and ReLU in the reduce kernel", bounds=_TINY),
    Case("fwd_gg_r32", "convUp", (32, 128, 9, 9, 32, 3, 3, 1, 1, 1), ("gg_kernel<1,4,1,128,rc,split>",), axis="channels", note="F <= 32", bounds=_TINY + _cancel_cap(0.7)),
    Case("fwd_gpw", "convUpBiasAct", (64, 128, 10, 10, 128, 3, 3, 1, 1, 1), (GPW,), relu=1, patch_mode=4, axis="channels", bounds=_TINY),
    Case("fwd_gpw_tail", "convUp", (128, 64, 27, 27, 256, 3, 3, 1, 1, 1), (GPW, "gg_tail_fix_kernel"), patch_mode=4, axis="channels",
         note="366 tiles on 256 slots: the last round cut in K"),
    Case("fwd_gpv", "convUp", (64, 16, 23, 23, 96, 5, 5, 2, 2, 0), ("gpv_kernel<96x512,split,raw>",), patch_mode=4, axis="channels"),
    Case("fwd_gpp_raw", "convUp", (64, 128, 9, 9, 128, 3, 3, 1, 1, 1), ("gpp_kernel<2,2,2,128,split,raw>",), patch_mode=1, axis="channels", bounds=_TINY),
    # ---- input gradient -----------------------------------------------------------------------------------------------------------
    Case("dgrad_ggp_s1", "convDown", (32, 128, 13, 13, 64, 3, 3, 1, 1, 1), (GG2,), axis="filters", note="conv3 type: stride 1", bounds=_TINY),
    Case("dgrad_classes_r128", "convDown", (32, 128, 13, 13, 256, 3, 3, 2, 2, 1), (GG2,), axis="filters", note="4 stride classes, one launch"),
    Case("dgrad_classes_r64", "convDown", (32, 64, 13, 13, 256, 3, 3, 2, 2, 1), (GG1,), axis="filters"),
    Case("dgrad_many_classes", "convDown", (32, 128, 20, 20, 512, 5, 5, 5, 5, 0), (GG2,), axis="filters",
         note="25 stride classes > kMaxClasses: one launch per class"),
    Case("dgrad_mask_wholek", "convDownMask", (32, 128, 13, 13, 64, 3, 3, 1, 1, 1), (GG2,), st=0.5, post_scale=2.0, axis="filters", bounds=_TINY),
    Case("dgrad_mask_tail", "convDownMask", (256, 256, 13, 13, 384, 3, 3, 1, 1, 1), (GG2, "gg_tail_fix_kernel"), post_scale=2.0,
         axis="filters", note="conv3 dgrad: 338 tiles on 256 slots", bounds=(('normal', (3.2, 1.0, 8.0)), ('huge', (3.7, 1.0, 8.0)), ('dynamic_range', (3.3, 2.0, 32.0)))),
    Case("dgrad_gpv_classes", "convDown", (64, 128, 19, 19, 128, 5, 5, 2, 2, 0), ("gpv_kernel<128x512,split,raw>",), patch_mode=4,
         axis="filters", bounds=_cancel_cap(0.6)),
    Case("dgrad_gpw", "convDown", (64, 128, 10, 10, 128, 3, 3, 1, 1, 1), (GPW,), patch_mode=4, axis="filters", bounds=_TINY),
    Case("dgrad_gpp_raw", "convDown", (64, 128, 9, 9, 64, 3, 3, 1, 1, 1), ("gpp_kernel<2,2,2,128,split,raw>",), patch_mode=1, axis="filters", bounds=_TINY),
    Case("dgrad_gpp_planes", "convDown", (64, 128, 9, 9, 64, 3, 3, 1, 1, 1), ("gpp_kernel<2,2,2,128,split,planes>",), patch_mode=2,
         axis="filters", bounds=_TINY),
    # ---- weight gradient ----------------------------------------------------------------------------------------------------------
    Case("wgrad_wg_128", "convOutpBias", (32, 32, 9, 9, 128, 3, 3, 1, 1, 1), ("wg_kernel<2,2,2,2,split>",), st=0.75, so=0.5, axis="images",
         note="K = 288: bias in the tile's spare row"),
    Case("wgrad_wg_x16", "convOutpBias", (32, 3, 15, 15, 96, 7, 7, 2, 2, 1), ("wg_kernel<2,2,5,3,x16,split>",), st=0.75, so=0.5, axis="images",
         note="conv1 type"),
    Case("wgrad_wg_96", "convOutpGemm", (32, 64, 9, 9, 96, 2, 2, 1, 1, 0), ("wg_kernel<4,1,1,3,split>",), axis="images"),
    Case("wgrad_wg_64", "convOutpGemm", (32, 64, 9, 9, 64, 2, 2, 1, 1, 0), ("wg_kernel<4,1,1,2,split>",), st=1.0, so=0.25, axis="images"),
    Case("wgrad_wg_32", "convOutpGemm", (32, 64, 9, 9, 32, 2, 2, 1, 1, 0), ("wg_kernel<4,1,1,1,split>",), axis="images"),
    Case("wgrad_reduce_two_level", "convOutpBias", (64, 16, 29, 29, 32, 3, 3, 1, 1, 0), ("wg_kernel<4,1,1,1,split>", "wg_reduce_kernel"),
         st=0.5, so=0.25, axis="images", note="2 tiles, 1458 chunks: 91 splits, the grouped reduce"),
    Case("wgrad_bias_fallback", "convOutpBias", (32, 32, 9, 9, 128, 2, 2, 1, 1, 0), ("wg_kernel<2,2,2,2,split>",), st=0.5, so=2.0,
         axis="images", note="K = 128 fills the tile: the bias gradient runs through sum_by_axis", bounds=(('normal', (2.4, 1.0, 8.0)),)),
    Case("wgrad_wgw", "convOutpBias", (32, 32, 9, 9, 256, 3, 3, 1, 1, 1), ("wgw_kernel<256x256,split>",), st=0.75, so=0.5, axis="images"),
    # ---- FC ------------------------------------------------------------------------------------------------------------------------
    Case("fc_nt_ggp", "dot", (256, 512, 256), ("ggp_kernel<2,2,2,128,split>",), trans="NT", axis="d"),
    Case("fc_nt_skinny", "dot", (64, 512, 256), ("gg_kernel<4,1,1,64,rc,split>",), trans="NT", axis="d", note="m <= 128", bounds=_TINY),
    Case("fc_nt_bias_relu", "dotBiasAct", (256, 512, 256), ("ggp_kernel<2,2,2,128,split>",), relu=1, trans="NT", axis="d"),
    Case("fc_nt_mask", "dotMask", (256, 512, 256), ("ggp_kernel<2,2,2,128,split>",), post_scale=2.0, trans="NT", axis="d"),
    Case("fc_nn_r128", "dot", (256, 256, 256), ("gg_kernel<2,2,2,128,kc,split>",), trans="NN", axis="f"),
    Case("fc_nn_r96", "dot", (256, 96, 256), ("gg_kernel<1,4,3,64,kc,split>",), st=0.5, trans="NN", axis="f"),
    Case("fc_nn_r64", "dot", (256, 64, 256), ("gg_kernel<2,2,1,128,kc,split>",), trans="NN", axis="f", bounds=_TINY),
    Case("fc_nn_r32", "dot", (256, 32, 256), ("gg_kernel<1,4,1,128,kc,split>",), trans="NN", axis="f"),
    Case("fc_nn_skinny", "dot", (64, 256, 256), ("gg_kernel<4,1,1,64,kc,split>",), trans="NN", axis="f"),
    Case("fc_nn_mask", "dotMask", (256, 256, 256), ("gg_kernel<2,2,2,128,kc,split>",), post_scale=2.0, trans="NN", axis="f"),
    Case("fc_tn_wg", "dot", (256, 256, 128), ("wg_kernel<2,2,2,2,split>",), st=0.75, so=0.5, trans="TN", axis="n"),
    Case("fc_tn_wg_96", "dot", (2048, 256, 96), ("wg_kernel<4,1,1,3,split>", "wg_reduce_kernel"), st=1.0, so=0.25, trans="TN", axis="n"),
    # ---- local ---------------------------------------------------------------------------------------------------------------------
    Case("local_face_up", "localUpBiasAct", (16, 16, 63, 63, 16, 9, 9, 1, 1, 0), ("lc_kernel<up,split>",), relu=1, axis="channels", bounds=_cancel_cap(1.4)),
    Case("local_face_down", "localDown", (16, 16, 63, 63, 16, 9, 9, 1, 1, 0), ("lc_kernel<down,split>",), st=0.5, axis="filters", bounds=_TINY + _cancel_cap(1.4)),
    Case("local_face_outp", "localOutp", (16, 16, 63, 63, 16, 9, 9, 1, 1, 0), ("lc_kernel<outp,split>",), st=0.75, so=0.5, axis="images", bounds=_cancel_cap(1.8)),
    Case("local_strided_up", "localUp", (64, 16, 11, 11, 32, 3, 3, 2, 2, 1), ("lc_kernel<up,split>",), st=0.5, axis="channels", bounds=_TINY + _cancel_cap(1.9)),
    Case("local_strided_bias", "localUpBiasAct", (64, 16, 11, 11, 32, 3, 3, 2, 2, 1), ("lc_kernel<up,split>",), relu=1, axis="channels", bounds=_cancel_cap(1.7) + (('normal', (2.0, 1.0, 8.0)),)),
    Case("local_strided_down", "localDown", (64, 16, 11, 11, 32, 3, 3, 2, 2, 1), ("lc_kernel<down,split>",), axis="filters", bounds=_TINY + _cancel_cap(0.7)),
    Case("local_strided_outp", "localOutp", (64, 16, 11, 11, 32, 3, 3, 2, 2, 1), ("lc_kernel<outp,split>",), so=0.5, axis="images"),
    # ---- launches that run the fp32 instruction on the split path too --------------------------------------------------------------
    Case("fallback_gg_nonvector", "convUp", (30, 128, 9, 9, 128, 3, 3, 1, 1, 1), ("gg_kernel<2,2,2,128,rc>",), fp32=True, axis="channels",
         note="N % 4 != 0: the scalar-load gg_kernel has no split build", bounds=_cancel_cap(0.8)),
    Case("fallback_dot_generic", "dot", (64, 256, 96), ("dot_generic_kernel",), so=0.5, trans="NT", fp32=True, axis="d",
         note="NT with alpha != 1 is not one of fc_edge.cc's shapes"),
]

# Kernel families with a split build (timer names with ",split", local_conv.hip's names[]) that have no row, and why.
EXEMPT = {}

# the families the CPU test looks for in the sources, by the timer-name prefix they carry
FAMILIES = ["gg_kernel", "ggp_kernel", "gpw_kernel", "gpv_kernel", "gpp_kernel", "wg_kernel", "wgw_kernel", "gfc_kernel", "lc_kernel"]


def family(name):
    return name.split("<", 1)[0]
