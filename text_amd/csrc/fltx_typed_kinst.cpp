/*
 * fltx_typed_kinst.cpp -- the kernels of fltx_decode_batch_typed (fltx_typed_entry.h: every dtype and kind), one object,
 * compiled without packed float32 instructions and linked into text_amd/lib/libfltx.so by __graft_entry__.build.
 */
#include "fltx_typed_entry.h"

#define FLTX_TYPED_INST(...) template __global__ void __VA_ARGS__;
FLTX_TYPED_ALL(FLTX_TYPED_INST)
#undef FLTX_TYPED_INST
