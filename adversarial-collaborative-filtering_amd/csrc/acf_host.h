// acf_host.h — host plumbing of the entry points of both libraries: libacf_apr.so (acf_apr.hip, training
// step; acf_plan.hip, its plan; acf_rank.hip, ranking family) and libacf_neumf.so (acf_neumf.hip, acf_keras_mf.hip): error macros,
// launch grid, row geometry, dim check, the kernels' range bits.  After hip_runtime.h, acf_apr.h.
#pragma once

// Each library has one thread-local error string and one definition of this function (acf_apr.hip,
// acf_neumf.hip).  Hidden: both libraries can be in one process, and an interposable symbol would send
// one library's messages to the string of whichever was loaded first; so each binds to its own copy.
__attribute__((visibility("hidden"))) int acf_set_error(int code, const char* fmt, ...);

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

// One float4 per lane (d <= 256): KFN<LPR> for the smallest power of two LPR with 4 LPR >= d.
#define DISPATCH_LPR(d, KFN, ...)                                                     \
  [&]() -> int {                                                                    \
    int lpr_ = 1;                                                                   \
    while (lpr_ * 4 < (d)) lpr_ <<= 1;                                              \
    switch (lpr_) {                                                                 \
      case 1: KFN<1>(__VA_ARGS__); break;                                           \
      case 2: KFN<2>(__VA_ARGS__); break;                                           \
      case 4: KFN<4>(__VA_ARGS__); break;                                           \
      case 8: KFN<8>(__VA_ARGS__); break;                                           \
      case 16: KFN<16>(__VA_ARGS__); break;                                         \
      case 32: KFN<32>(__VA_ARGS__); break;                                         \
      case 64: KFN<64>(__VA_ARGS__); break;                                         \
      default: return acf_set_error(ACF_E_INVALID, "unsupported dim %d", (int)(d)); \
    }                                                                               \
    return ACF_OK;                                                                  \
  }()

// The error word the kernels of libacf_neumf.so set: bit 1 a user index, bit 2 an item index outside its
// table (the kernel used row 0 instead).
static inline int range_err(int32_t herr) {
  ACF_CHECK(herr == 0, ACF_E_RANGE, "index out of range (%s%s)", (herr & 1) ? "user >= num_user_rows " : "",
            (herr & 2) ? "item >= num_item_rows" : "");
  return ACF_OK;
}

// ... read back from the device once stream s has run dry
static inline int read_range_err(const int32_t* err, hipStream_t s) {
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return range_err(herr);
}

static inline int check_dim(int d) {
  ACF_CHECK(d >= 4 && d <= 1024 && d % 4 == 0, ACF_E_INVALID,
            "dim must be a multiple of 4 in [4, 1024], got %d", d);
  return ACF_OK;
}
