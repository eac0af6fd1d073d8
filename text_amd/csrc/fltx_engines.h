/*
 * fltx_engines.h -- the compiled geometries of every lane engine, one X-macro list per family.
 *
 *   fltx_instances.h            instantiates the kernels from these lists,
 *   kLaneKernels (fltx_api.cpp) maps each (family, variant, geometry) to its kernel -- and, in the emulator
 *                               build (tests/emu), to the host function of the same source,
 *   prepare() (fltx_api.cpp)    chooses among their rows.
 *
 * A geometry is added here and nowhere else.
 */
#pragma once

/* FLTX_ROW(X, ROW): X applied to the fields of a row that is one macro (the token-LM mlane rows below) */
#define FLTX_ROW(X, ...) X(__VA_ARGS__)

/* fltx_slane.h, lane = LM state, and its token-LM variant (tlane): X(threads, list positions per token wave).  Two of
 * the waves do not evaluate tokens (own groups of the lanes / row staging and housekeeping). */
#define FLTX_SLANE_GEOS(X) X(320, 10) X(384, 7) X(448, 6) X(512, 5) X(576, 4) X(640, 4) X(512, 12) X(576, 10)
/* ... the tlane rows with a phase-clock variant (bench.py --profile) */
#define FLTX_TLANE_PROF_GEOS(X) X(576, 4) X(512, 5)
/* ... a stream's chunks (slane_stream / tlane_stream), in order of preference */
#define FLTX_SSTREAM_GEOS(X) X(576, 4) X(512, 5) X(576, 10)

/* fltx_mlane.h, several lane groups: X(threads, list positions per wave and group, lane groups, groups per token wave,
 * groups per self wave).  The row number is the "mlane_geo" tunable: keep the order. */
#define FLTX_MLANE_GEOS(X)                                                                                         \
  X(640, 4, 2, 2, 1) X(960, 5, 2, 1, 1) X(640, 10, 2, 2, 1) X(768, 4, 4, 4, 1) X(960, 5, 4, 2, 2) X(960, 11, 4, 2, 2) \
  X(960, 10, 8, 2, 4)
/* ... its token-LM variant (tmlane), in order of preference; one row per translation unit (fltx_instances.h) */
#define FLTX_TMLANE_GEO0 960, 5, 2, 1, 1
#define FLTX_TMLANE_GEO1 960, 11, 2, 1, 1
#define FLTX_TMLANE_GEO2 960, 5, 4, 2, 2
#define FLTX_TMLANE_GEO3 960, 11, 4, 2, 2
#define FLTX_TMLANE_GEO4 960, 10, 8, 2, 4
#define FLTX_TMLANE_GEOS(X)                                                                                          \
  FLTX_ROW(X, FLTX_TMLANE_GEO0) FLTX_ROW(X, FLTX_TMLANE_GEO1) FLTX_ROW(X, FLTX_TMLANE_GEO2)                        \
  FLTX_ROW(X, FLTX_TMLANE_GEO3) FLTX_ROW(X, FLTX_TMLANE_GEO4)

/* fltx_wlane.h, token beams over large token sets: X(threads, list positions per wave) */
#define FLTX_WLANE_GEOS(X) X(576, 5) X(576, 8) X(576, 10)

/* fltx_xlane.h, lane = (LM state, trie node): X(threads, list positions per wave), in order of preference; three waves
 * do not evaluate listed tokens */
#define FLTX_XLANE_GEOS(X) X(512, 2) X(512, 3) X(640, 2) X(576, 5) X(640, 10)

/* fltx_ylane.h, with the LM terms: X(threads, lane groups, rounds, memo in HBM = shares a CU, ...) rows, each compiled
 * for pairs of LM-term variants LMK (bit 0 LM terms, 1 ASG, 2 several words per spelling, 3 logAdd):
 *   FLTX_YLANE_GEOS, FLTX_YLANE4_GEOS:  LMK (0, 1) (2, 3) (8, 9) (10, 11); a phase-clock variant of (0, 1) on the first
 *   FLTX_YLANE_MULTI_GEOS:              LMK (5, 7) (13, 15) (memo in HBM: the larger merge table takes its place) */
#define FLTX_YLANE_GEOS(X, ...) \
  X(512, 1, 2, 0, __VA_ARGS__) X(768, 2, 4, 0, __VA_ARGS__) X(512, 1, 2, 1, __VA_ARGS__) X(512, 2, 4, 1, __VA_ARGS__)
/* four lane groups (beams 129 .. 256): ten token waves, four for the lanes' own groups, the word and staging waves */
#define FLTX_YLANE4_GEOS(X, ...) X(1024, 4, 4, 1, __VA_ARGS__)
#define FLTX_YLANE_MULTI_GEOS(X, ...) X(512, 1, 2, 1, __VA_ARGS__) X(768, 2, 4, 1, __VA_ARGS__)
/* K(threads, groups, rounds, memo in HBM, LMK) over one row and LMK pair */
#define FLTX_YLMK_01(W, NG, R, HM, K) K(W, NG, R, HM, 0) K(W, NG, R, HM, 1)
#define FLTX_YLMK_23(W, NG, R, HM, K) K(W, NG, R, HM, 2) K(W, NG, R, HM, 3)
#define FLTX_YLMK_89(W, NG, R, HM, K) K(W, NG, R, HM, 8) K(W, NG, R, HM, 9)
#define FLTX_YLMK_1011(W, NG, R, HM, K) K(W, NG, R, HM, 10) K(W, NG, R, HM, 11)
#define FLTX_YLMK_57(W, NG, R, HM, K) K(W, NG, R, HM, 5) K(W, NG, R, HM, 7)
#define FLTX_YLMK_1315(W, NG, R, HM, K) K(W, NG, R, HM, 13) K(W, NG, R, HM, 15)
#define FLTX_YLMK_PLAIN(W, NG, R, HM, K) \
  FLTX_YLMK_01(W, NG, R, HM, K) FLTX_YLMK_23(W, NG, R, HM, K) FLTX_YLMK_89(W, NG, R, HM, K) FLTX_YLMK_1011(W, NG, R, HM, K)
#define FLTX_YLMK_MULTI(W, NG, R, HM, K) FLTX_YLMK_57(W, NG, R, HM, K) FLTX_YLMK_1315(W, NG, R, HM, K)
/* every compiled fltx_ylane.h kernel: K(threads, groups, rounds, memo in HBM, LMK) */
#define FLTX_YLANE_KERNELS(K) \
  FLTX_YLANE_GEOS(FLTX_YLMK_PLAIN, K) FLTX_YLANE4_GEOS(FLTX_YLMK_PLAIN, K) FLTX_YLANE_MULTI_GEOS(FLTX_YLMK_MULTI, K)
