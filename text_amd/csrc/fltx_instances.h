/*
 * fltx_instances.h -- every decode-kernel instantiation the host can launch
 * (launchDecode in fltx_api.cpp), as FLTX_INST(name<args>) lines grouped so
 * that one group of one workgroup size is one translation unit.
 *
 *   fltx_api.cpp    : no FLTX_INST_W  -> all groups x all sizes (extern template)
 *   fltx_kinst.cpp  : -DFLTX_INST_W=512 -DFLTX_INST_G=1 -> that group only
 *
 * (No include guard: it is included with different FLTX_INST definitions.)
 */
#define FLTX_G1(W) /* lane-per-slot step, 4 tokens per wave */ \
  FLTX_INST(fltx_decode_kernel_lane<W, 4, false, false>)      \
  FLTX_INST(fltx_decode_kernel_lane<W, 4, false, true>)       \
  FLTX_INST(fltx_decode_kernel_lane<W, 4, true, false>)       \
  FLTX_INST(fltx_decode_kernel_lane<W, 4, true, true>)
#define FLTX_G2(W) /* lane-per-slot step, 8 tokens per wave */ \
  FLTX_INST(fltx_decode_kernel_lane<W, 8, false, false>)      \
  FLTX_INST(fltx_decode_kernel_lane<W, 8, false, true>)       \
  FLTX_INST(fltx_decode_kernel_lane<W, 8, true, false>)       \
  FLTX_INST(fltx_decode_kernel_lane<W, 8, true, true>)
#define FLTX_G3(W) /* lean step, groups in registers / streaming */ \
  FLTX_INST(fltx_decode_kernel_lds<W, 6>)                          \
  FLTX_INST(fltx_decode_kernel_lds<W, 12>)                         \
  FLTX_INST(fltx_decode_kernel_lds<W, 255>)
#define FLTX_G4(W) FLTX_INST(fltx_decode_kernel_lds<W, 0>) /* generic engine */
#define FLTX_G5(W) FLTX_INST(fltx_decode_kernel_lds_spec<W, true, true>)
#define FLTX_G6(W) FLTX_INST(fltx_decode_kernel_lds_spec<W, true, false>)
#define FLTX_G7(W) FLTX_INST(fltx_decode_kernel_lds_spec<W, false, true>)
#define FLTX_G8(W) FLTX_INST(fltx_decode_kernel_gws<W>)
#define FLTX_G9(W) FLTX_INST(fltx_decode_kernel_gwslean<W>)
/* the lane engines: the geometries of fltx_engines.h, one group per (family, variant) -- or per row where a kernel is
 * large; W is ignored */
#include "fltx_engines.h"
#define FLTX_I_SLANE(WW, GG, LA, PROF) FLTX_INST(fltx_decode_kernel_slane<WW, GG, LA, PROF>)
#define FLTX_I_SLANE_M32(WW, GG, PROF) FLTX_INST(fltx_decode_kernel_slane<WW, GG, false, PROF, true>)
#define FLTX_I_TLANE(WW, GG, ...) FLTX_INST(fltx_decode_kernel_tlane<WW, GG, __VA_ARGS__>)
#define FLTX_I_SSTREAM(WW, GG) FLTX_INST(fltx_decode_kernel_slane_stream<WW, GG>)
#define FLTX_I_TSTREAM(WW, GG) FLTX_INST(fltx_decode_kernel_tlane_stream<WW, GG>)
#define FLTX_I_MLANE(WW, GG, NG, GPW, SPW, LA) FLTX_INST(fltx_decode_kernel_mlane<WW, GG, NG, GPW, SPW, LA>)
#define FLTX_I_XLANE(WW, GG, ...) FLTX_INST(fltx_decode_kernel_xlane<WW, GG, __VA_ARGS__>)
#define FLTX_I_WLANE(WW, GG) FLTX_INST(fltx_decode_kernel_wlane<WW, GG>)
#define FLTX_I_YLANE(WW, NG, RR, HM, LMK) FLTX_INST(fltx_decode_kernel_ylane<WW, NG, RR, LMK, HM, false>)
#define FLTX_I_YLANE_PROF(WW, NG, RR, HM, LMK) FLTX_INST(fltx_decode_kernel_ylane<WW, NG, RR, LMK, HM, true>)
#define FLTX_I_TMLANE(LA, ...) FLTX_INST(fltx_decode_kernel_tmlane<__VA_ARGS__, LA>)
#define FLTX_G10(W) FLTX_SLANE_GEOS(FLTX_I_SLANE_PLAIN)
#define FLTX_I_SLANE_PLAIN(WW, GG) FLTX_I_SLANE(WW, GG, false, false)
#define FLTX_G11(W) FLTX_SLANE_GEOS(FLTX_I_SLANE_PROF)
#define FLTX_I_SLANE_PROF(WW, GG) FLTX_I_SLANE(WW, GG, false, true)
#define FLTX_G41(W) FLTX_SLANE_GEOS(FLTX_I_SLANE_PLAIN32) /* 32-bit token masks: at most 32 tokens */
#define FLTX_I_SLANE_PLAIN32(WW, GG) FLTX_I_SLANE_M32(WW, GG, false)
#define FLTX_G42(W) FLTX_SLANE_GEOS(FLTX_I_SLANE_PROF32)
#define FLTX_I_SLANE_PROF32(WW, GG) FLTX_I_SLANE_M32(WW, GG, true)
#define FLTX_G15(W) FLTX_SLANE_GEOS(FLTX_I_SLANE_LA) /* logAdd */
#define FLTX_I_SLANE_LA(WW, GG) FLTX_I_SLANE(WW, GG, true, false)
#define FLTX_G28(W) FLTX_SLANE_GEOS(FLTX_I_TLANE_PLAIN) FLTX_TLANE_PROF_GEOS(FLTX_I_TLANE_PROF)
#define FLTX_I_TLANE_PLAIN(WW, GG) FLTX_I_TLANE(WW, GG, false)
#define FLTX_I_TLANE_PROF(WW, GG) FLTX_I_TLANE(WW, GG, false, true)
#define FLTX_G29(W) FLTX_SLANE_GEOS(FLTX_I_TLANE_LA) /* logAdd */
#define FLTX_I_TLANE_LA(WW, GG) FLTX_I_TLANE(WW, GG, true)
#define FLTX_G16(W) FLTX_SSTREAM_GEOS(FLTX_I_SSTREAM)
#define FLTX_G30(W) FLTX_SSTREAM_GEOS(FLTX_I_TSTREAM)
#define FLTX_G18(W) FLTX_MLANE_GEOS(FLTX_I_MLANE_MAX)
#define FLTX_I_MLANE_MAX(WW, GG, NG, GPW, SPW) FLTX_I_MLANE(WW, GG, NG, GPW, SPW, false)
#define FLTX_G19(W) FLTX_MLANE_GEOS(FLTX_I_MLANE_LA) /* logAdd */
#define FLTX_I_MLANE_LA(WW, GG, NG, GPW, SPW) FLTX_I_MLANE(WW, GG, NG, GPW, SPW, true)
#define FLTX_G31(W) FLTX_I_TMLANE(false, FLTX_TMLANE_GEO0)
#define FLTX_G32(W) FLTX_I_TMLANE(false, FLTX_TMLANE_GEO2)
#define FLTX_G33(W) FLTX_I_TMLANE(false, FLTX_TMLANE_GEO4)
#define FLTX_G34(W) FLTX_I_TMLANE(false, FLTX_TMLANE_GEO1)
#define FLTX_G35(W) FLTX_I_TMLANE(false, FLTX_TMLANE_GEO3)
#define FLTX_G36(W) FLTX_I_TMLANE(true, FLTX_TMLANE_GEO0) /* logAdd */
#define FLTX_G37(W) FLTX_I_TMLANE(true, FLTX_TMLANE_GEO2)
#define FLTX_G38(W) FLTX_I_TMLANE(true, FLTX_TMLANE_GEO4)
#define FLTX_G39(W) FLTX_I_TMLANE(true, FLTX_TMLANE_GEO1)
#define FLTX_G40(W) FLTX_I_TMLANE(true, FLTX_TMLANE_GEO3)
#define FLTX_G22(W) FLTX_WLANE_GEOS(FLTX_I_WLANE)
#define FLTX_G12(W) FLTX_XLANE_GEOS(FLTX_I_XLANE_PLAIN) FLTX_XLANE_GEOS(FLTX_I_XLANE_PROF)
#define FLTX_I_XLANE_PLAIN(WW, GG) FLTX_I_XLANE(WW, GG, 0, false)
#define FLTX_I_XLANE_PROF(WW, GG) FLTX_I_XLANE(WW, GG, 0, true)
#define FLTX_G17(W) FLTX_XLANE_GEOS(FLTX_I_XLANE_HBM) /* memo in HBM: shares a CU */
#define FLTX_I_XLANE_HBM(WW, GG) FLTX_I_XLANE(WW, GG, 1, false)
#define FLTX_G24(W) FLTX_XLANE_GEOS(FLTX_I_XLANE_LA) FLTX_XLANE_GEOS(FLTX_I_XLANE_LA_HBM) /* logAdd */
#define FLTX_I_XLANE_LA(WW, GG) FLTX_I_XLANE(WW, GG, 0, false, true)
#define FLTX_I_XLANE_LA_HBM(WW, GG) FLTX_I_XLANE(WW, GG, 1, false, true)
#define FLTX_G13(W) FLTX_YLANE_GEOS(FLTX_YLMK_01, FLTX_I_YLANE)
#define FLTX_G14(W) FLTX_YLANE_GEOS(FLTX_YLMK_01, FLTX_I_YLANE_PROF)
#define FLTX_G20(W) FLTX_YLANE4_GEOS(FLTX_YLMK_01, FLTX_I_YLANE) FLTX_YLANE4_GEOS(FLTX_YLMK_23, FLTX_I_YLANE)
#define FLTX_G21(W) FLTX_YLANE_GEOS(FLTX_YLMK_23, FLTX_I_YLANE) /* ASG */
#define FLTX_G23(W) FLTX_YLANE_MULTI_GEOS(FLTX_YLMK_57, FLTX_I_YLANE)
#define FLTX_G25(W) FLTX_YLANE_GEOS(FLTX_YLMK_89, FLTX_I_YLANE) FLTX_YLANE4_GEOS(FLTX_YLMK_89, FLTX_I_YLANE) /* logAdd */
#define FLTX_G26(W) FLTX_YLANE_GEOS(FLTX_YLMK_1011, FLTX_I_YLANE) FLTX_YLANE4_GEOS(FLTX_YLMK_1011, FLTX_I_YLANE)
#define FLTX_G27(W) FLTX_YLANE_MULTI_GEOS(FLTX_YLMK_1315, FLTX_I_YLANE)

#ifdef FLTX_INST_W
#define FLTX_CAT2_(a, b) a##b
#define FLTX_CAT_(a, b) FLTX_CAT2_(a, b)
FLTX_CAT_(FLTX_G, FLTX_INST_G)(FLTX_INST_W)
#undef FLTX_CAT_
#undef FLTX_CAT2_
#else
#define FLTX_ALLG(W) FLTX_G1(W) FLTX_G2(W) FLTX_G3(W) FLTX_G4(W) FLTX_G5(W) FLTX_G6(W) FLTX_G7(W) FLTX_G8(W) FLTX_G9(W)
FLTX_ALLG(64)
FLTX_ALLG(128)
FLTX_ALLG(256)
FLTX_ALLG(512)
FLTX_ALLG(1024)
FLTX_G10(0)
FLTX_G11(0)
FLTX_G12(0)
FLTX_G13(0)
FLTX_G14(0)
FLTX_G15(0)
FLTX_G16(0)
FLTX_G17(0)
FLTX_G18(0)
FLTX_G19(0)
FLTX_G20(0)
FLTX_G21(0)
FLTX_G22(0)
FLTX_G23(0)
FLTX_G24(0)
FLTX_G25(0)
FLTX_G26(0)
FLTX_G27(0)
FLTX_G28(0)
FLTX_G29(0)
FLTX_G30(0)
FLTX_G31(0)
FLTX_G32(0)
FLTX_G33(0)
FLTX_G34(0)
FLTX_G35(0)
FLTX_G36(0)
FLTX_G37(0)
FLTX_G38(0)
FLTX_G39(0)
FLTX_G40(0)
FLTX_G41(0)
FLTX_G42(0)
#undef FLTX_ALLG
#endif
#undef FLTX_G1
#undef FLTX_G2
#undef FLTX_G3
#undef FLTX_G4
#undef FLTX_G5
#undef FLTX_G6
#undef FLTX_G7
#undef FLTX_G8
#undef FLTX_G9
#undef FLTX_G10
#undef FLTX_G11
#undef FLTX_G12
#undef FLTX_G13
#undef FLTX_G14
#undef FLTX_G15
#undef FLTX_G16
#undef FLTX_G17
#undef FLTX_G18
#undef FLTX_G19
#undef FLTX_G20
#undef FLTX_G21
#undef FLTX_G22
#undef FLTX_G23
#undef FLTX_G24
#undef FLTX_G31
#undef FLTX_G32
#undef FLTX_G33
#undef FLTX_G34
#undef FLTX_G35
#undef FLTX_G36
#undef FLTX_G37
#undef FLTX_G38
#undef FLTX_G39
#undef FLTX_G40
#undef FLTX_G41
#undef FLTX_G42
#undef FLTX_G25
#undef FLTX_G26
#undef FLTX_G27
#undef FLTX_G28
#undef FLTX_G29
#undef FLTX_G30
#undef FLTX_I_SLANE
#undef FLTX_I_SLANE_M32
#undef FLTX_I_TLANE
#undef FLTX_I_SSTREAM
#undef FLTX_I_TSTREAM
#undef FLTX_I_MLANE
#undef FLTX_I_XLANE
#undef FLTX_I_WLANE
#undef FLTX_I_YLANE
#undef FLTX_I_YLANE_PROF
#undef FLTX_I_TMLANE
