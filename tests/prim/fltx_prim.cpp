/*
 * tests/prim/fltx_prim.cpp -- small kernels around the lane engines' selection primitives, for
 * tests/test_selection_primitives.py.  TEST INFRASTRUCTURE ONLY: nothing in text_amd/ loads it.
 *
 * Every body calls the product headers' helpers as they are (fltx_slane.h, fltx_wlane.h, fltx_rt.h); one
 * configuration per workgroup, so that one launch covers thousands of them.  Two builds of this source:
 *   HIP (__graft_entry__.build(), HIP_FLAGS)  -> tests/prim/libfltx_prim.so      the code that ships, on the GPU
 *   FLTX_EMU (g++ + tests/emu/hip_emu.cpp)    -> tests/prim/libfltx_prim_emu.so  the same bodies on the emulator
 * Every entry point is extern "C", takes host arrays, does its own allocation, copies, launch and synchronisation,
 * and returns the HIP status (0 = success; the emulator always returns 0).
 */
#include <cstdio> /* (before fltx_kernels.h: fltx_ylane.h writes to stderr) */
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fltx_kernels.h"
#include "fltx_engines.h"

using namespace fltx;

/* ---- host side: device buffers and launches -------------------------------------------------------------------- */
namespace {
struct Dev {
  std::vector<void*> ptrs;
  int st = 0;
  void* alloc(size_t bytes) {
    void* p = nullptr;
    bytes = bytes ? bytes : 8;
#ifdef FLTX_EMU
    p = calloc(1, bytes);
    st = st ? st : (p ? 0 : 2);
#else
    if (st == 0) {
      st = (int)hipMalloc(&p, bytes);
    }
    if (st == 0) {
      st = (int)hipMemset(p, 0, bytes);
    }
#endif
    if (p) {
      ptrs.push_back(p);
    }
    return p;
  }
  template <class T>
  T* in(const T* h, size_t n) {
    T* d = (T*)alloc(n * sizeof(T));
#ifdef FLTX_EMU
    if (d) {
      memcpy(d, h, n * sizeof(T));
    }
#else
    if (st == 0) {
      st = (int)hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
    }
#endif
    return d;
  }
  template <class T>
  T* out(size_t n) {
    return (T*)alloc(n * sizeof(T));
  }
  template <class T>
  void back(T* h, const T* d, size_t n) {
#ifdef FLTX_EMU
    if (st == 0) {
      memcpy(h, d, n * sizeof(T));
    }
#else
    if (st == 0) {
      st = (int)hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    }
#endif
  }
  ~Dev() {
    for (void* p : ptrs) {
#ifdef FLTX_EMU
      free(p);
#else
      (void)hipFree(p);
#endif
    }
  }
};
} // namespace

#ifdef FLTX_EMU
/* BODY(args, smem) on nBlocks workgroups of W threads */
#define PRIM_LAUNCH(KERNEL, BODY, nBlocks, W, lds, A, dev)                                       \
  do {                                                                                           \
    if ((dev).st == 0 && (nBlocks) > 0) {                                                        \
      const auto a_ = (A);                                                                       \
      emuLaunch((nBlocks), (W), (lds), [&a_](char* smem) { BODY(a_, smem); });                  \
    }                                                                                            \
  } while (0)
#else
#define PRIM_LAUNCH(KERNEL, BODY, nBlocks, W, lds, A, dev)                                       \
  do {                                                                                           \
    if ((dev).st == 0 && (nBlocks) > 0) {                                                        \
      hipLaunchKernelGGL(KERNEL, dim3((unsigned)(nBlocks)), dim3((unsigned)(W)), (lds), 0, (A)); \
      (dev).st = (int)hipGetLastError();                                                         \
      if ((dev).st == 0) {                                                                       \
        (dev).st = (int)hipStreamSynchronize(0);                                                 \
      }                                                                                          \
    }                                                                                            \
  } while (0)
#endif

/* ================================================================================================================
 * slRankBin<NJ>: the members of the boundary bin, published by atomAdd in arbitrary order as the callers do.
 * Configuration c: cnt members (slot = (wave * NJ + j) * 64 + lane, key), need; nUsed < NJ: the ylane predicate
 * shape `j < nUsed && ...`, with every slot j >= nUsed of every lane in the bin but not a member.
 * Output: every thread's `take`.
 * ================================================================================================================ */
struct RankArgs {
  const int32_t* cfg;              /* [nCfg][3]: cnt, need, nUsed */
  const uint32_t* slot;            /* [nCfg][kSlBCap] */
  const unsigned long long* key;   /* [nCfg][kSlBCap] */
  uint32_t* take;                  /* [nCfg][W] */
};
struct RankLds {
  unsigned long long bKey[kSlBCap];
  uint32_t bOrd[kSlBCap];
  uint32_t n;
};
template <int NJ>
FLTX_DEV void rankBody(const RankArgs& A, char* smem) {
  RankLds& S = *(RankLds*)smem;
  const int c = (int)blockIdx.x, lane = laneId();
  const int wave = waveUniform(waveId());
  const int W = (int)blockDim.x;
  const int cnt = A.cfg[3 * c], need = A.cfg[3 * c + 1], nUsed = A.cfg[3 * c + 2];
  bool inBin[NJ];
  unsigned long long k[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const uint32_t me = (uint32_t)((wave * NJ + j) * 64 + lane);
    inBin[j] = j >= nUsed; /* (not a member: the caller's predicate leaves these out) */
    k[j] = 0x9E3779B97F4A7C15ull * (me + 1u); /* (what a non-member holds must not matter) */
    for (int i = 0; i < cnt; ++i) {
      if (A.slot[c * kSlBCap + i] == me) {
        inBin[j] = true;
        k[j] = A.key[c * kSlBCap + i];
      }
    }
  }
  if (threadIdx.x == 0) {
    S.n = 0u;
  }
  ldsBarrier();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j < nUsed && inBin[j]) {
      const uint32_t i = atomAdd32(&S.n, 1u);
      S.bKey[i] = k[j];
      S.bOrd[i] = ((uint32_t)wave << 16) | ((uint32_t)j << 8) | (uint32_t)lane;
    }
  }
  ldsBarrier();
  const uint32_t take = slRankBin<NJ>(S.bKey, S.bOrd, cnt, need, wave, [&](int j) { return j < nUsed && inBin[j]; },
                                      [&](int j) { return k[j]; });
  A.take[(size_t)c * W + threadIdx.x] = take;
}

#ifndef FLTX_EMU
template <int W, int NJ>
__global__ void __launch_bounds__(W) prim_rank_kernel(RankArgs A) {
  extern __shared__ __attribute__((aligned(16))) char prim_smem[];
  rankBody<NJ>(A, prim_smem);
}
/* the same body with the scalar registers cut to 24: its frame loop spills SGPRs, as fltx_wlane.h's does
 * (test_selection_primitives.py checks that the built object reports the spills) */
template <int W, int NJ>
__global__ void __launch_bounds__(W) __attribute__((amdgpu_num_sgpr(24))) prim_rank_spill_kernel(RankArgs A) {
  extern __shared__ __attribute__((aligned(16))) char prim_smem[];
  rankBody<NJ>(A, prim_smem);
}
#endif

/* every (threads, NJ) pair a caller of slRankBin compiles, from fltx_engines.h:
 *   slane / tlane  (threads, GT)              mlane / tmlane  (threads, GT * GPW)
 *   xlane          (threads, GT)              ylane           (threads, NS: NS0 = max(R, NG, 2); word wave NG + 2 NG)
 *   wlane          (threads, GT): the variant it does not use today */
#define PRIM_SL(W, GT) X(W, GT)
#define PRIM_ML(W, GT, NG, GPW, SPW) X(W, GT * GPW)
#define PRIM_YL_NS0(W, NG, R) ((R) > (NG) ? (R) : ((NG) > 2 ? (NG) : 2))
#define PRIM_YL(W, NG, R, HM, ...) X(W, PRIM_YL_NS0(W, NG, R))
#define PRIM_YLM(W, NG, R, HM, ...) X(W, PRIM_YL_NS0(W, NG, R)) X(W, (NG) + 2 * (NG))
#define PRIM_RANK_PAIRS                                                                                    \
  FLTX_SLANE_GEOS(PRIM_SL) FLTX_MLANE_GEOS(PRIM_ML) FLTX_TMLANE_GEOS(PRIM_ML) FLTX_XLANE_GEOS(PRIM_SL)      \
  FLTX_YLANE_GEOS(PRIM_YL, 0) FLTX_YLANE4_GEOS(PRIM_YL, 0) FLTX_YLANE_MULTI_GEOS(PRIM_YLM, 0)               \
  FLTX_WLANE_GEOS(PRIM_SL)

/* the pairs, in the order of the list (duplicates included): a test enumerates them */
extern "C" int prim_rank_pairs(int32_t* out, int cap) {
  int n = 0;
#define X(W, NJ)         \
  if (n < cap) {         \
    out[2 * n] = (W);    \
    out[2 * n + 1] = (NJ); \
  }                      \
  ++n;
  PRIM_RANK_PAIRS
#undef X
  return n;
}

/* spill: 1 = the SGPR-pressure kernel (one pair only: 576 threads, NJ = 10, wlane's widest) */
extern "C" int prim_rank(int W, int NJ, int spill, int nCfg, const int32_t* cfg, const uint32_t* slot,
                         const unsigned long long* key, uint32_t* take) {
  Dev dev;
  RankArgs A;
  A.cfg = dev.in(cfg, (size_t)nCfg * 3);
  A.slot = dev.in(slot, (size_t)nCfg * kSlBCap);
  A.key = dev.in(key, (size_t)nCfg * kSlBCap);
  A.take = dev.out<uint32_t>((size_t)nCfg * W);
  bool found = false;
  if (spill) {
    if (W == 576 && NJ == 10) {
      found = true;
      PRIM_LAUNCH((prim_rank_spill_kernel<576, 10>), rankBody<10>, nCfg, 576, sizeof(RankLds), A, dev);
    }
  } else {
#define X(W_, NJ_)                                                                                  \
  if (!found && W == (W_) && NJ == (NJ_)) {                                                         \
    found = true;                                                                                   \
    PRIM_LAUNCH((prim_rank_kernel<(W_), (NJ_)>), rankBody<(NJ_)>, nCfg, (W_), sizeof(RankLds), A, dev); \
  }
    PRIM_RANK_PAIRS
#undef X
  }
  if (!found) {
    return -1;
  }
  dev.back(take, A.take, (size_t)nCfg * W);
  return dev.st;
}

/* ================================================================================================================
 * slScan(hist, K, noFar): one wave per configuration, the histogram staged in LDS as the callers keep it.
 * Output per configuration: bstar, cum, cnt, total, crossed.
 * ================================================================================================================ */
struct ScanArgs {
  const uint32_t* hist; /* [nCfg][kSlNB] */
  const int32_t* kf;    /* [nCfg][2]: K, noFar */
  int32_t* out;         /* [nCfg][5] */
};
FLTX_DEV void scanBody(const ScanArgs& A, char* smem) {
  uint32_t* h = (uint32_t*)smem;
  const int c = (int)blockIdx.x, lane = laneId();
  for (int i = lane; i < kSlNB; i += 64) {
    h[i] = A.hist[(size_t)c * kSlNB + i];
  }
  waveSync();
  const SlScan r = slScan(h, A.kf[2 * c], A.kf[2 * c + 1] != 0);
  if (lane == 0) {
    int32_t* o = A.out + 5 * c;
    o[0] = r.bstar;
    o[1] = r.cum;
    o[2] = r.cnt;
    o[3] = r.total;
    o[4] = r.crossed ? 1 : 0;
  }
}
#ifndef FLTX_EMU
__global__ void __launch_bounds__(64) prim_scan_kernel(ScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) char prim_smem[];
  scanBody(A, prim_smem);
}
#endif
extern "C" int prim_scan(int nCfg, const uint32_t* hist, const int32_t* kf, int32_t* out) {
  Dev dev;
  ScanArgs A;
  A.hist = dev.in(hist, (size_t)nCfg * kSlNB);
  A.kf = dev.in(kf, (size_t)nCfg * 2);
  A.out = dev.out<int32_t>((size_t)nCfg * 5);
  PRIM_LAUNCH(prim_scan_kernel, scanBody, nCfg, 64, kSlNB * 4, A, dev);
  dev.back(out, A.out, (size_t)nCfg * 5);
  return dev.st;
}

/* ================================================================================================================
 * slBin<false> and slBin<true>, slLogAdd, f64Key / f32Key: elementwise, 64 elements per workgroup.
 * ================================================================================================================ */
struct BinArgs {
  const double* best;
  const double* c;
  const int32_t* sb; /* [n][2]: shift, base */
  int32_t* out;      /* [n][2]: slBin<false>, slBin<true> */
  int n;
};
FLTX_DEV void binBody(const BinArgs& A, char*) {
  const int i = (int)blockIdx.x * 64 + laneId();
  if (i < A.n) {
    A.out[2 * i] = slBin<false>(A.best[i], A.c[i], A.sb[2 * i], A.sb[2 * i + 1]);
    A.out[2 * i + 1] = slBin<true>(A.best[i], A.c[i], A.sb[2 * i], A.sb[2 * i + 1]);
  }
}
#ifndef FLTX_EMU
__global__ void __launch_bounds__(64) prim_bin_kernel(BinArgs A) { binBody(A, nullptr); }
#endif
extern "C" int prim_bin(int n, const double* best, const double* c, const int32_t* sb, int32_t* out) {
  Dev dev;
  BinArgs A;
  A.best = dev.in(best, (size_t)n);
  A.c = dev.in(c, (size_t)n);
  A.sb = dev.in(sb, (size_t)n * 2);
  A.out = dev.out<int32_t>((size_t)n * 2);
  A.n = n;
  PRIM_LAUNCH(prim_bin_kernel, binBody, (n + 63) / 64, 64, 0, A, dev);
  dev.back(out, A.out, (size_t)n * 2);
  return dev.st;
}

struct LogAddArgs {
  const double* hi;
  const double* lo;
  double* out;
  int n;
};
FLTX_DEV void logAddBody(const LogAddArgs& A, char*) {
  const int i = (int)blockIdx.x * 64 + laneId();
  if (i < A.n) {
    A.out[i] = slLogAdd(A.hi[i], A.lo[i]);
  }
}
#ifndef FLTX_EMU
__global__ void __launch_bounds__(64) prim_logadd_kernel(LogAddArgs A) { logAddBody(A, nullptr); }
#endif
extern "C" int prim_logadd(int n, const double* hi, const double* lo, double* out) {
  Dev dev;
  LogAddArgs A;
  A.hi = dev.in(hi, (size_t)n);
  A.lo = dev.in(lo, (size_t)n);
  A.out = dev.out<double>((size_t)n);
  A.n = n;
  PRIM_LAUNCH(prim_logadd_kernel, logAddBody, (n + 63) / 64, 64, 0, A, dev);
  dev.back(out, A.out, (size_t)n);
  return dev.st;
}

struct KeyArgs {
  const double* d;
  const float* f;
  unsigned long long* k64; /* [n][2]: f64Key(d), bits of f64FromKey(f64Key(d)) */
  uint32_t* k32;           /* [n][2]: f32Key(f), bits of f32FromKey(f32Key(f)) */
  int n;
};
FLTX_DEV void keyBody(const KeyArgs& A, char*) {
  const int i = (int)blockIdx.x * 64 + laneId();
  if (i < A.n) {
    const unsigned long long k = f64Key(A.d[i]);
    A.k64[2 * i] = k;
    A.k64[2 * i + 1] = (unsigned long long)__double_as_longlong(f64FromKey(k));
    const uint32_t k32 = f32Key(A.f[i]);
    A.k32[2 * i] = k32;
    A.k32[2 * i + 1] = __float_as_uint(f32FromKey(k32));
  }
}
#ifndef FLTX_EMU
__global__ void __launch_bounds__(64) prim_key_kernel(KeyArgs A) { keyBody(A, nullptr); }
#endif
extern "C" int prim_keys(int n, const double* d, const float* f, unsigned long long* k64, uint32_t* k32) {
  Dev dev;
  KeyArgs A;
  A.d = dev.in(d, (size_t)n);
  A.f = dev.in(f, (size_t)n);
  A.k64 = dev.out<unsigned long long>((size_t)n * 2);
  A.k32 = dev.out<uint32_t>((size_t)n * 2);
  A.n = n;
  PRIM_LAUNCH(prim_key_kernel, keyBody, (n + 63) / 64, 64, 0, A, dev);
  dev.back(k64, A.k64, (size_t)n * 2);
  dev.back(k32, A.k32, (size_t)n * 2);
  return dev.st;
}

/* ================================================================================================================
 * The wave primitives: one wave per configuration.  In: 64 u64 per lane-row, a per-lane source lane, a uniform mask
 * and xor distance.  Out per lane (kWaveOut u64): waveInclusiveScan (of the low 31 bits), waveMax64, waveMax32 (of the
 * low 32 bits), waveMin64, wavePrefixCount, waveShfl64, waveShflXor64, waveRowRor64<0..15>.
 * ================================================================================================================ */
constexpr int kWaveOut = 7 + 16;
struct WaveArgs {
  const unsigned long long* v;   /* [nCfg][64] */
  const int32_t* src;            /* [nCfg][64] */
  const unsigned long long* mm;  /* [nCfg][2]: mask, xor distance */
  unsigned long long* out;       /* [nCfg][kWaveOut][64] */
};
template <int R>
FLTX_DEV void rorAll(unsigned long long v, unsigned long long* o) {
  if constexpr (R < 16) {
    o[R * 64] = waveRowRor64<R>(v);
    rorAll<R + 1>(v, o);
  }
}
FLTX_DEV void waveBody(const WaveArgs& A, char*) {
  const int c = (int)blockIdx.x, lane = laneId();
  const unsigned long long v = A.v[(size_t)c * 64 + lane];
  const int src = A.src[(size_t)c * 64 + lane];
  const unsigned long long m = A.mm[2 * c];
  const int x = (int)A.mm[2 * c + 1];
  unsigned long long* o = A.out + (size_t)c * kWaveOut * 64 + lane;
  o[0 * 64] = (unsigned long long)(uint32_t)waveInclusiveScan((int)(v & 0x7FFFFFFFull));
  o[1 * 64] = waveMax64(v);
  o[2 * 64] = waveMax32((uint32_t)v);
  o[3 * 64] = waveMin64(v);
  o[4 * 64] = (unsigned long long)wavePrefixCount(m);
  o[5 * 64] = waveShfl64(v, src);
  o[6 * 64] = waveShflXor64(v, x);
  rorAll<0>(v, o + 7 * 64);
}
#ifndef FLTX_EMU
__global__ void __launch_bounds__(64) prim_wave_kernel(WaveArgs A) { waveBody(A, nullptr); }
#endif
extern "C" int prim_wave(int nCfg, const unsigned long long* v, const int32_t* src, const unsigned long long* mm,
                         unsigned long long* out) {
  Dev dev;
  WaveArgs A;
  A.v = dev.in(v, (size_t)nCfg * 64);
  A.src = dev.in(src, (size_t)nCfg * 64);
  A.mm = dev.in(mm, (size_t)nCfg * 2);
  A.out = dev.out<unsigned long long>((size_t)nCfg * kWaveOut * 64);
  PRIM_LAUNCH(prim_wave_kernel, waveBody, nCfg, 64, 0, A, dev);
  dev.back(out, A.out, (size_t)nCfg * kWaveOut * 64);
  return dev.st;
}

/* ================================================================================================================
 * slRowScan (slane's token beam and the frame's best candidate): one wave per configuration; lane n holds e[n] (the
 * lanes past N hold whatever the row array has there -- they must not matter).
 * Out: allow, listMask, bits of best, ekey, nList, dead, bits of esil.
 * ================================================================================================================ */
struct RowArgs {
  const int32_t* cfg;  /* [nCfg][5]: N, Kt, sil, blank, ctc */
  const double* sc;    /* [nCfg][2]: mmax, silScore */
  const float* row;    /* [nCfg][64] */
  unsigned long long* out; /* [nCfg][7] */
};
FLTX_DEV void rowBody(const RowArgs& A, char*) {
  const int c = (int)blockIdx.x, lane = laneId();
  DecodeParams P; /* (slRowScan reads N, Kt, sil and blank) */
  P.N = A.cfg[5 * c];
  P.Kt = A.cfg[5 * c + 1];
  P.sil = A.cfg[5 * c + 2];
  P.blank = A.cfg[5 * c + 3];
  const bool ctc = A.cfg[5 * c + 4] != 0;
  const SlRowRegs r = slRowScan(P, A.row[(size_t)c * 64 + lane], ctc, A.sc[2 * c], A.sc[2 * c + 1]);
  if (lane == 0) {
    unsigned long long* o = A.out + 7 * c;
    o[0] = r.allow;
    o[1] = r.listMask;
    o[2] = (unsigned long long)__double_as_longlong(r.best);
    o[3] = r.ekey;
    o[4] = (unsigned long long)(uint32_t)r.nList;
    o[5] = r.dead ? 1ull : 0ull;
    o[6] = __float_as_uint(r.esil);
  }
}
#ifndef FLTX_EMU
__global__ void __launch_bounds__(64) prim_row_kernel(RowArgs A) { rowBody(A, nullptr); }
#endif
extern "C" int prim_rowscan(int nCfg, const int32_t* cfg, const double* sc, const float* row, unsigned long long* out) {
  Dev dev;
  RowArgs A;
  A.cfg = dev.in(cfg, (size_t)nCfg * 5);
  A.sc = dev.in(sc, (size_t)nCfg * 2);
  A.row = dev.in(row, (size_t)nCfg * 64);
  A.out = dev.out<unsigned long long>((size_t)nCfg * 7);
  PRIM_LAUNCH(prim_row_kernel, rowBody, nCfg, 64, 0, A, dev);
  dev.back(out, A.out, (size_t)nCfg * 7);
  return dev.st;
}

/* ================================================================================================================
 * wlTokBeamRows (fltx_wlane.h's front end) over B utterances of T rows of N emissions, launched as fltx_api.cpp
 * launches it (grid tokRowBlocks * B, four waves, four WlFrontLds).  Out: the WlTokRow records, row = b * T + t.
 * ================================================================================================================ */
static_assert(sizeof(WlTokRow) == 416, "the test reads 416-byte records");
#ifndef FLTX_EMU
__global__ void __launch_bounds__(256) prim_tokbeam_kernel(DecodeParams P) {
  extern __shared__ __attribute__((aligned(16))) char prim_smem[];
  wlTokBeamRows(P, prim_smem);
}
#endif
FLTX_DEV void tokBeamBody(const DecodeParams& P, char* smem) { wlTokBeamRows(P, smem); }
extern "C" int prim_tokbeam(int B, int T, int N, int Kt, int criterion, int blank, int sil, const float* em,
                            void* rows) {
  Dev dev;
  const int K = 8; /* (the beam: only histOff / K is read) */
  std::vector<int64_t> emOff((size_t)B), histOff((size_t)B);
  std::vector<int32_t> stepT((size_t)B, T);
  for (int b = 0; b < B; ++b) {
    emOff[(size_t)b] = (int64_t)b * T * N;
    histOff[(size_t)b] = (int64_t)b * T * K;
  }
  DecodeParams P;
  memset((void*)&P, 0, sizeof(P));
  P.N = N;
  P.Kt = Kt;
  P.K = K;
  P.criterion = criterion;
  P.blank = blank;
  P.sil = sil;
  P.emissions = dev.in(em, (size_t)B * T * N);
  P.emOff = dev.in(emOff.data(), (size_t)B);
  P.histOff = dev.in(histOff.data(), (size_t)B);
  P.stepT = dev.in(stepT.data(), (size_t)B);
  P.uttMap = nullptr;
  P.tokRows = dev.out<WlTokRow>((size_t)B * T);
  P.tokRowBlocks = (T + 3) / 4 > 1 ? (T + 3) / 4 : 1; /* (fltx_api.cpp: max(1, (wlMaxT + 3) / 4)) */
  PRIM_LAUNCH(prim_tokbeam_kernel, tokBeamBody, P.tokRowBlocks * B, 256, 4 * sizeof(WlFrontLds), P, dev);
  dev.back((WlTokRow*)rows, (const WlTokRow*)P.tokRows, (size_t)B * T);
  return dev.st;
}

extern "C" int prim_wl_tokrow_size() { return (int)sizeof(WlTokRow); }
