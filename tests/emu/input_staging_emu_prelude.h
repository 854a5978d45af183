// Force-included in front of convnet_amd/csrc/input_staging.hip when tests/test_input_staging_emulated.py compiles it as host C++: what
// that file needs beyond tests/emu/hip/hip_runtime.h.  A static __shared__ array is one array per block there (blocks run one after the
// other on one OS thread, so a function-local static serves), and the kernels clamp 64-bit indices with min / max.
#pragma once
#include <hip/hip_runtime.h>
#undef __shared__
#define __shared__ static
inline long min(long a, long b) { return a < b ? a : b; }
inline long max(long a, long b) { return a > b ? a : b; }
inline long long min(long long a, long long b) { return a < b ? a : b; }
inline long long max(long long a, long long b) { return a > b ? a : b; }
