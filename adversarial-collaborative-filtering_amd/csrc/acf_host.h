// acf_host.h — host plumbing of the entry points in acf_apr.hip (training engine) and acf_rank.hip
// (ranking family): error macros, launch grid, row geometry, dim check.  After hip_runtime.h, acf_apr.h.
#pragma once

// The library's one thread-local error string and this function's one definition are in acf_apr.hip.
int acf_set_error(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess)                                                      \
      return acf_set_error(ACF_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

#define ACF_CHECK(cond, code, ...)                                             \
  do {                                                                         \
    if (!(cond)) return acf_set_error((code), __VA_ARGS__);                    \
  } while (0)

#define ACF_RET(x)                  \
  do {                              \
    int r_ = (x);                   \
    if (r_ != ACF_OK) return r_;    \
  } while (0)

static inline unsigned grid_for(int64_t n, int bs = 256) {
  return (unsigned)((n + bs - 1) / bs);
}

// Row-group geometry for a given dim: LPR lanes per row, NV float4 per lane.
static inline void geometry(int d, int* lpr, int* nv) {
  int d4 = d / 4;
  int l = 1;
  while (l < d4 && l < 64) l <<= 1;
  *lpr = l;
  *nv = (d4 + l - 1) / l;
}

#define DISPATCH_GEOM(d, KFN, ...)                                                    \
  [&]() -> int {                                                                    \
    int lpr_, nv_;                                                                  \
    geometry((d), &lpr_, &nv_);                                                     \
    switch (lpr_ * 100 + nv_) {                                                     \
      case 101: KFN<1, 1>(__VA_ARGS__); break;                                      \
      case 201: KFN<2, 1>(__VA_ARGS__); break;                                      \
      case 401: KFN<4, 1>(__VA_ARGS__); break;                                      \
      case 801: KFN<8, 1>(__VA_ARGS__); break;                                      \
      case 1601: KFN<16, 1>(__VA_ARGS__); break;                                    \
      case 3201: KFN<32, 1>(__VA_ARGS__); break;                                    \
      case 6401: KFN<64, 1>(__VA_ARGS__); break;                                    \
      case 6402: KFN<64, 2>(__VA_ARGS__); break;                                    \
      case 6403: KFN<64, 3>(__VA_ARGS__); break;                                    \
      case 6404: KFN<64, 4>(__VA_ARGS__); break;                                    \
      default: return acf_set_error(ACF_E_INVALID, "unsupported dim %d", (int)(d)); \
    }                                                                               \
    return ACF_OK;                                                                  \
  }()

static inline int check_dim(int d) {
  ACF_CHECK(d >= 4 && d <= 1024 && d % 4 == 0, ACF_E_INVALID,
            "dim must be a multiple of 4 in [4, 1024], got %d", d);
  return ACF_OK;
}
