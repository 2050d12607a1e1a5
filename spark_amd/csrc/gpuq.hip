/*
 * gpuq.hip — MI355X-native (gfx950, CDNA4) kernels behind the gpuq C-ABI.
 *
 * Everything here is HBM-bandwidth-bound integer/hash work (no MFMA — there
 * is no dense contraction on this path): design centers on
 * coalesced 64-lane access, LDS digit histograms, wave-wide ballot
 * multi-split ranking, and device-scope atomics.
 *
 * Reference semantics restated (cites into /root/reference):
 *  - LSB radix sort, 8-bit digits, skip-uniform-bytes:
 *    core/.../unsafe/sort/RadixSort.java:43-139 — here as a stable
 *    three-kernel pass (per-block histogram, global exclusive scan over
 *    [bin][block], ranked scatter through LDS staging).
 *  - sort-key encodings: PrefixComparators.java:66-83 (double bijection),
 *    SignedPrefixComparator (two's-complement order == unsigned order with
 *    the sign bit flipped). Descending = stable ascending radix on the
 *    bitwise complement (order-equivalent to RadixSort's desc bucket walk).
 *  - Murmur3_x86_32: common/unsafe/.../hash/Murmur3_x86_32.java:45-147.
 *  - partition id: Pmod(Murmur3Hash(key,42), n), partitioning.scala:328-330.
 *  - hash aggregate / hash join: observable semantics of
 *    HashAggregateExec + BytesToBytesMap and ShuffledHashJoinExec +
 *    LongHashedRelation (open addressing; duplicates chained) — GPU-native
 *    linear probing with device-scope atomics, not a translation.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

#include "../../include/gpuq.h"

/* ================= error machinery ================= */

static __thread char g_err[512];

extern "C" const char* gpuq_last_error(void) { return g_err; }

#define FAIL(code, ...) do { \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__); return (code); } while (0)

#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    snprintf(g_err, sizeof(g_err), "%s failed: %s (%s:%d)", #expr, \
             hipGetErrorString(_e), __FILE__, __LINE__); \
    return GPUQ_ERR_HIP; } } while (0)

extern "C" int gpuq_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

/* ---- optional per-kernel HIP-event profiling (bench roofline) ----
 * Events are recorded on the launching stream around individual kernel
 * launches; gpuq_kernel_stats() drains (synchronizes) and accumulates. */
#include <vector>
#include <map>
#include <string>
#include <mutex>

static std::mutex g_prof_mu;
static bool g_prof_on = false;
struct prof_rec { const char* tag; hipEvent_t a, b; };
static std::vector<prof_rec> g_prof_pending;
static std::map<std::string, std::pair<double, long long>> g_prof_acc;

extern "C" void gpuq_profiling(int enable) { g_prof_on = enable != 0; }

static hipEvent_t prof_begin(hipStream_t s) {
  if (!g_prof_on) return nullptr;
  hipEvent_t e; (void)hipEventCreate(&e); (void)hipEventRecord(e, s);
  return e;
}
static void prof_end(const char* tag, hipStream_t s, hipEvent_t a) {
  if (!a) return;
  hipEvent_t b; (void)hipEventCreate(&b); (void)hipEventRecord(b, s);
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_prof_pending.push_back({tag, a, b});
}

extern "C" void gpuq_kernel_stats_reset(void) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  for (auto& r : g_prof_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  g_prof_pending.clear();
  g_prof_acc.clear();
}

extern "C" int gpuq_kernel_stats(const char* name, double* total_ms, long long* count) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  for (auto& r : g_prof_pending) {
    (void)hipEventSynchronize(r.b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    auto& acc = g_prof_acc[r.tag];
    acc.first += ms; acc.second += 1;
    (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
  }
  g_prof_pending.clear();
  auto it = g_prof_acc.find(name);
  if (it == g_prof_acc.end()) { *total_ms = 0; *count = 0; return GPUQ_OK; }
  *total_ms = it->second.first;
  *count = it->second.second;
  return GPUQ_OK;
}

/* ================= device inlines ================= */

#define WAVE 64
#define DEV static __device__ __forceinline__

DEV uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

/* Murmur3_x86_32.java:125-147 */
DEV uint32_t mm3_mixK1(uint32_t k1) {
  k1 *= 0xcc9e2d51u; k1 = rotl32(k1, 15); k1 *= 0x1b873593u; return k1;
}
DEV uint32_t mm3_mixH1(uint32_t h1, uint32_t k1) {
  h1 ^= k1; h1 = rotl32(h1, 13); return h1 * 5u + 0xe6546b64u;
}
DEV uint32_t mm3_fmix(uint32_t h1, uint32_t len) {
  h1 ^= len; h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13;
  h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16; return h1;
}
/* Murmur3_x86_32.java:109-122 hashLong */
DEV int32_t mm3_hash_long(int64_t input, int32_t seed) {
  uint32_t lo = (uint32_t)(uint64_t)input;
  uint32_t hi = (uint32_t)((uint64_t)input >> 32);
  uint32_t h1 = mm3_mixH1((uint32_t)seed, mm3_mixK1(lo));
  h1 = mm3_mixH1(h1, mm3_mixK1(hi));
  return (int32_t)mm3_fmix(h1, 8);
}
/* Pmod (catalyst arithmetic.scala Pmod.pmod for int) */
DEV int32_t spark_pmod(int32_t a, int32_t n) {
  int32_t r = a % n; return r < 0 ? r + n : r;
}

/* splitmix64 — bit-identical to oracle/oracle.c gen_u64 */
DEV uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}
DEV uint64_t gen_u64_dev(uint64_t seed, uint64_t i) {
  return splitmix64(seed * 0x9E3779B97F4A7C15ULL + i);
}

#define SIGNBIT 0x8000000000000000ULL

/* PrefixComparators.java:72-83 DoublePrefixComparator.computePrefix */
DEV uint64_t encode_f64(double v) {
  if (v == -0.0) v = 0.0;
  uint64_t bits;
  if (v != v) bits = 0x7ff8000000000000ULL;  /* Java canonical NaN */
  else bits = __double_as_longlong(v);
  uint64_t mask = (uint64_t)(-(int64_t)(bits >> 63)) | SIGNBIT;
  return bits ^ mask;
}
/* SignedPrefixComparator order == unsigned order with sign flipped */
DEV uint64_t encode_i64(int64_t v) { return (uint64_t)v ^ SIGNBIT; }

/* inverses of the monotone encodings (also used by MIN/MAX accumulators,
 * which hold encoded u64 so atomicMin/atomicMax give the right order) */
DEV int64_t decode_i64(uint64_t e) { return (int64_t)(e ^ SIGNBIT); }
DEV double decode_f64(uint64_t e) {
  uint64_t mask = ((e >> 63) ? 0 : ~0ULL) | SIGNBIT;
  return __longlong_as_double((long long)(e ^ mask));
}

/* sort output word for an encoded key: decode_mode 0 keeps the encoded key,
 * 1 = int64, 2 = float64, +4 = the key was complemented for DESC. Shared by
 * the fused final scatter pass and the tie-fix kernel. */
DEV uint64_t sort_out_word(uint64_t kk, int decode_mode) {
  if (!decode_mode) return kk;
  uint64_t e = (decode_mode & 4) ? ~kk : kk;
  if (decode_mode & 2) {
    uint64_t mask = ((e >> 63) ? 0 : ~0ULL) | SIGNBIT;
    return e ^ mask;
  }
  return e ^ SIGNBIT;
}

/* sort input word for a raw key: the inverse direction of sort_out_word.
 * in_mode 0 = the word is already encoded, 1 = int64, 2 = float64 (-0.0 ->
 * +0.0, canonical NaN: encode_f64), +4 = complement for DESC. Used by the
 * fused first scatter pass, which reads the caller's column directly. */
DEV uint64_t sort_in_word(uint64_t raw, int in_mode) {
  if (!in_mode) return raw;
  uint64_t e = (in_mode & 2) ? encode_f64(__longlong_as_double((long long)raw))
                             : encode_i64((int64_t)raw);
  return (in_mode & 4) ? ~e : e;
}

DEV bool bit_valid(const uint8_t* validity, int64_t i) {
  return !validity || ((validity[i >> 3] >> (i & 7)) & 1);
}

/* ================= synthetic data generation ================= */

__global__ void k_gen_i64_range(uint64_t seed, uint64_t start, int64_t n,
                                uint64_t range, int64_t* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t v = gen_u64_dev(seed, start + (uint64_t)i);
    out[i] = (int64_t)(range ? v % range : v);
  }
}

__global__ void k_gen_f64_unit(uint64_t seed, uint64_t start, int64_t n, double* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t v = gen_u64_dev(seed, start + (uint64_t)i);
    out[i] = (double)(v >> 11) * (1.0 / 9007199254740992.0);
  }
}

/* grid shape for random-access hash kernels (A/B via GPUQ_HASH_GRID:
 * 0 = one element per thread, N = cap at N blocks with grid-stride) */
static dim3 hash_grid(int64_t n, int block = 256) {
  static int cap = -2;
  if (cap == -2) {
    const char* e = getenv("GPUQ_HASH_GRID");
    cap = e ? atoi(e) : 2048;
  }
  int64_t b = (n + block - 1) / block;
  if (cap > 0 && b > cap) b = cap;
  if (b > 0x7FFFFFFF) b = 0x7FFFFFFF;
  if (b < 1) b = 1;
  return dim3((uint32_t)b);
}

static dim3 grid1d(int64_t n, int block = 256) {
  int64_t b = (n + block - 1) / block;
  if (b > 2048) b = 2048;  /* grid-stride beyond (G11: cap + stride) */
  if (b < 1) b = 1;
  return dim3((uint32_t)b);
}

extern "C" int gpuq_gen_i64_range(void* stream, uint64_t seed, uint64_t start,
                                  int64_t n, uint64_t range, int64_t* out) {
  k_gen_i64_range<<<grid1d(n), 256, 0, (hipStream_t)stream>>>(seed, start, n, range, out);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

extern "C" int gpuq_gen_f64_unit(void* stream, uint64_t seed, uint64_t start,
                                 int64_t n, double* out) {
  k_gen_f64_unit<<<grid1d(n), 256, 0, (hipStream_t)stream>>>(seed, start, n, out);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ================= gather ================= */

template <typename T>
__global__ void k_gather(int64_t n, const T* in, const uint32_t* perm, T* out) {
  /* 4-way unrolled so four independent random loads are in flight per lane
   * (random gathers are latency-bound; same lesson as the scatter preload) */
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    uint32_t p0 = perm[i], p1 = perm[i + stride], p2 = perm[i + 2 * stride],
             p3 = perm[i + 3 * stride];
    T v0 = in[p0], v1 = in[p1], v2 = in[p2], v3 = in[p3];
    out[i] = v0; out[i + stride] = v1;
    out[i + 2 * stride] = v2; out[i + 3 * stride] = v3;
  }
  for (; i < n; i += stride) out[i] = in[perm[i]];
}

/* two columns through one permutation (both payload gathers of a sort step
 * in one kernel: one perm read, two independent random loads in flight) */
__global__ void k_gather2(int64_t n, const uint64_t* a, const uint64_t* b,
                          const uint32_t* perm, uint64_t* oa, uint64_t* ob) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < n; i += 2 * stride) {
    uint32_t p0 = perm[i], p1 = perm[i + stride];
    uint64_t a0 = a[p0], b0 = b[p0], a1 = a[p1], b1 = b[p1];
    oa[i] = a0; ob[i] = b0;
    oa[i + stride] = a1; ob[i + stride] = b1;
  }
  for (; i < n; i += stride) {
    uint32_t p = perm[i];
    oa[i] = a[p]; ob[i] = b[p];
  }
}

extern "C" int gpuq_gather2_i64(void* stream, int64_t n, const void* a,
                                const void* b, const uint32_t* perm,
                                void* oa, void* ob) {
  { hipEvent_t _pe = prof_begin((hipStream_t)stream);
  k_gather2<<<grid1d(n), 256, 0, (hipStream_t)stream>>>(
      n, (const uint64_t*)a, (const uint64_t*)b, perm,
      (uint64_t*)oa, (uint64_t*)ob);
  prof_end("gather2", (hipStream_t)stream, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ---- interleaved two-column gather ----
 * The plain two-column gather issues 2 random 8 B loads per row; each
 * touches a 64 B line, so the fetch amplification is ~5x and the kernel
 * saturates on request rate (round-1 PMC: 39 B fetched per 8 B row).
 * Interleaving the source columns into 16 B records first (one streaming
 * pass) halves the random request count and doubles bytes-per-line used:
 * one b128 load serves both columns. */

__global__ void k_interleave2(int64_t n, const uint64_t* a, const uint64_t* b,
                              ulonglong2* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) {
    ulonglong2 v;
    v.x = a[i];
    v.y = b[i];
    out[i] = v;
  }
}

__global__ void k_gather2_pairs(int64_t n, const ulonglong2* pairs,
                                const uint32_t* perm, uint64_t* oa,
                                uint64_t* ob) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) {
    ulonglong2 v = pairs[perm[i]];
    oa[i] = v.x;
    ob[i] = v.y;
  }
}

/* 4-way batched variant: each thread keeps 4 independent b128 loads in
 * flight (A/B vs the scalar grid-stride loop; selected by env). */
__global__ void k_gather2_pairs4(int64_t n, const ulonglong2* pairs,
                                 const uint32_t* perm, uint64_t* oa,
                                 uint64_t* ob) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t base = t * 4; base < n; base += stride) {
    uint32_t p[4];
    ulonglong2 v[4];
    int top = (int)((n - base) < 4 ? (n - base) : 4);
    #pragma unroll
    for (int q = 0; q < 4; q++)
      if (q < top) p[q] = perm[base + q];
    #pragma unroll
    for (int q = 0; q < 4; q++)
      if (q < top) v[q] = pairs[p[q]];
    #pragma unroll
    for (int q = 0; q < 4; q++)
      if (q < top) {
        oa[base + q] = v[q].x;
        ob[base + q] = v[q].y;
      }
  }
}

extern "C" int gpuq_interleave2_i64(void* stream, int64_t n, const void* a,
                                    const void* b, void* pairs) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return GPUQ_OK;
  { hipEvent_t _pe = prof_begin(s);
  k_interleave2<<<grid1d(n), 256, 0, s>>>(n, (const uint64_t*)a,
                                          (const uint64_t*)b,
                                          (ulonglong2*)pairs);
  prof_end("interleave2", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

extern "C" int gpuq_gather2_pairs(void* stream, int64_t n, const void* pairs,
                                  const uint32_t* perm, void* oa, void* ob) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return GPUQ_OK;
  static int mlp0 = -1;
  if (mlp0 < 0) mlp0 = getenv("GPUQ_GATHER_MLP") ? atoi(getenv("GPUQ_GATHER_MLP")) : 0;
  { hipEvent_t _pe = prof_begin(s);
  if (mlp0)
    k_gather2_pairs4<<<grid1d((n + 3) / 4), 256, 0, s>>>(
        n, (const ulonglong2*)pairs, perm, (uint64_t*)oa, (uint64_t*)ob);
  else
    k_gather2_pairs<<<grid1d(n), 256, 0, s>>>(n, (const ulonglong2*)pairs,
                                              perm, (uint64_t*)oa,
                                              (uint64_t*)ob);
  prof_end("gather2_pairs", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* scratch: n * 16 bytes, device. */
extern "C" int gpuq_gather2_i64_fast(void* stream, int64_t n, const void* a,
                                     const void* b, const uint32_t* perm,
                                     void* oa, void* ob, void* scratch) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return GPUQ_OK;
  { hipEvent_t _pe = prof_begin(s);
  k_interleave2<<<grid1d(n), 256, 0, s>>>(n, (const uint64_t*)a,
                                          (const uint64_t*)b,
                                          (ulonglong2*)scratch);
  prof_end("interleave2", s, _pe); }
  HIP_TRY(hipGetLastError());
  static int mlp = -1;
  if (mlp < 0) mlp = getenv("GPUQ_GATHER_MLP") ? atoi(getenv("GPUQ_GATHER_MLP")) : 0;
  { hipEvent_t _pe = prof_begin(s);
  if (mlp)
    k_gather2_pairs4<<<grid1d((n + 3) / 4), 256, 0, s>>>(
        n, (const ulonglong2*)scratch, perm, (uint64_t*)oa, (uint64_t*)ob);
  else
    k_gather2_pairs<<<grid1d(n), 256, 0, s>>>(n, (const ulonglong2*)scratch,
                                              perm, (uint64_t*)oa,
                                              (uint64_t*)ob);
  prof_end("gather2_pairs", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

extern "C" int gpuq_gather(void* stream, int64_t n, gpuq_col col,
                           const uint32_t* perm, void* out) {
  hipStream_t s = (hipStream_t)stream;
  if (col.dtype == GPUQ_INT64 || col.dtype == GPUQ_FLOAT64) {
    k_gather<uint64_t><<<grid1d(n, 256), 256, 0, s>>>(n, (const uint64_t*)col.data, perm, (uint64_t*)out);
  } else if (col.dtype == GPUQ_INT32) {
    k_gather<uint32_t><<<grid1d(n, 256), 256, 0, s>>>(n, (const uint32_t*)col.data, perm, (uint32_t*)out);
  } else {
    FAIL(GPUQ_ERR_INVALID, "gather: unsupported dtype %d", col.dtype);
  }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ================= radix sort / partition machinery ================= */
/*
 * Stable LSB radix over 8-bit digits on (u64 key, u32 rowid) pairs.
 * Per pass: per-block 256-bin histogram -> global exclusive scan over the
 * [bin][block] matrix (bin-major => stable (bin, block, in-block) order) ->
 * ranked scatter. In-block stable ranks come from a wave-level ballot
 * multi-split (8 ballots reconstruct the same-digit lane mask), wave-private
 * LDS counters, then a cross-wave/cross-bin LDS scan; the tile is staged
 * reordered through LDS so global writes go out as contiguous digit runs
 * (coalesced except run boundaries).
 */

#define SORT_BLOCK 256
#define SORT_WAVES (SORT_BLOCK / WAVE)
#define SORT_ITEMS 16
#define SORT_TILE (SORT_BLOCK * SORT_ITEMS) /* 4096 */

/* encode kernel: keys -> radix-encoded u64 + identity rowids + bitwise
 * AND/OR reduction for the skip-uniform-byte decision (RadixSort.java:113-124) */
/* encode + identity rowids + skip-byte AND/OR reduction + ALL EIGHT global
 * byte histograms in one read (one pass replaces the reference's per-byte
 * count loops, RadixSort.java:126-135; per-byte histograms are invariant
 * under the passes' permutations, so one upfront count serves every pass).
 * Histogram-only mode (ek == idx == nullptr, no rowmap): the reduction and
 * the histograms over keys encoded in registers, nothing materialised — the
 * pre-pass of the fused first scatter pass. Four keys per thread are in
 * flight per iteration there (measured against one key per thread, wave-
 * private and lane-interleaved histogram copies and contiguous tiles:
 * profiles/README.md, "Fused first pass"). */
template <int DTYPE, bool DESC>
__global__ void k_encode(int64_t n, const void* keys, const uint32_t* rowmap,
                         uint64_t* ek, uint32_t* idx,
                         unsigned long long* bits_and, unsigned long long* bits_or,
                         uint32_t* ghist /* [8][256] */) {
  __shared__ uint32_t h[8][256];
  for (int b = threadIdx.x; b < 8 * 256; b += blockDim.x) ((uint32_t*)h)[b] = 0;
  __syncthreads();
  uint64_t acc_or = 0, acc_and = ~0ULL;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (!ek) {
    for (; i + 3 * stride < n; i += 4 * stride) {
      uint64_t e[4];
      #pragma unroll
      for (int u = 0; u < 4; u++) {
        if (DTYPE == GPUQ_FLOAT64) e[u] = encode_f64(((const double*)keys)[i + u * stride]);
        else e[u] = encode_i64(((const int64_t*)keys)[i + u * stride]);
        if (DESC) e[u] = ~e[u];
      }
      #pragma unroll
      for (int u = 0; u < 4; u++) {
        acc_or |= e[u]; acc_and &= e[u];
        #pragma unroll
        for (int b = 0; b < 8; b++) atomicAdd(&h[b][(e[u] >> (b * 8)) & 0xff], 1u);
      }
    }
  }
  for (; i < n; i += stride) {
    uint64_t e;
    uint32_t row = rowmap ? rowmap[i] : (uint32_t)i;
    if (DTYPE == GPUQ_FLOAT64) e = encode_f64(((const double*)keys)[row]);
    else e = encode_i64(((const int64_t*)keys)[row]);
    if (DESC) e = ~e;
    if (ek) {
      ek[i] = e;
      idx[i] = row;
    }
    acc_or |= e; acc_and &= e;
    #pragma unroll
    for (int b = 0; b < 8; b++) atomicAdd(&h[b][(e >> (b * 8)) & 0xff], 1u);
  }
  /* wave reduce then one atomic per wave (G12) */
  for (int off = 32; off > 0; off >>= 1) {
    acc_or |= __shfl_down((unsigned long long)acc_or, off);
    acc_and &= __shfl_down((unsigned long long)acc_and, off);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    atomicOr(bits_or, (unsigned long long)acc_or);
    atomicAnd(bits_and, (unsigned long long)acc_and);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 8 * 256; b += blockDim.x) {
    uint32_t v = ((uint32_t*)h)[b];
    if (v) atomicAdd(&ghist[b], v);
  }
}

/* ---- ranked scatter pass ----
 * BIN_MODE 0: digit = (key >> shift) & 0xff  (radix sort pass)          */
struct scatter_geom { int block, items; };
static scatter_geom get_sort_geom(void);

template <int BIN_MODE>
DEV int compute_bin(uint64_t key, int shift, int nparts) {
  (void)nparts;
  if (BIN_MODE == 0) return (int)((key >> shift) & 0xff);
  /* BIN_MODE 3: byte `shift/8` of the TOP-16 murmur bits (two stable
   * passes order rows by a 16-bit hash bucket — partitioned aggregation) */
  return (int)((((uint32_t)mm3_hash_long((int64_t)key, 42)) >> (16 + shift)) & 0xff);
}

/* validity split for sort-with-nulls: pair key = 0 for the group that
 * sorts first (nulls when nulls_first), 1 for the other; also counts the
 * null rows (SortExec null ordering, SortOrder.scala:35-45) */
__global__ void k_validity_pids(int64_t n, const uint8_t* validity, int nulls_first,
                                uint64_t* pid_as_key, uint32_t* idx,
                                unsigned long long* null_count) {
  __shared__ unsigned int h;
  if (threadIdx.x == 0) h = 0;
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int mine = 0;
  for (; i < n; i += stride) {
    bool valid = (validity[i >> 3] >> (i & 7)) & 1;
    pid_as_key[i] = (uint64_t)(valid == (bool)nulls_first);
    idx[i] = (uint32_t)i;
    if (!valid) mine++;
  }
  if (mine) atomicAdd(&h, mine);
  __syncthreads();
  if (threadIdx.x == 0 && h) atomicAdd(null_count, (unsigned long long)h);
}

/* per-block histogram of digit at `shift` over the pass input;
 * `tile` elements per block (must match the scatter geometry) */
template <int BIN_MODE>
__global__ void k_radix_hist(int64_t n, const uint64_t* keys, int shift,
                             uint32_t* hist /* [256][nblocks] */, int nblocks,
                             int tile) {
  __shared__ uint32_t h[256];
  if (threadIdx.x < 256) h[threadIdx.x] = 0;
  __syncthreads();
  int64_t base = (int64_t)blockIdx.x * tile;
  int rounds = tile / 256;
  for (int r = 0; r < rounds; r++) {
    int64_t i = base + r * 256 + threadIdx.x;
    if (i < n) atomicAdd(&h[compute_bin<BIN_MODE>(keys[i], shift, 0)], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 256)
    hist[(int64_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

/* ---- generic exclusive scan over uint32 (for the hist matrix) ---- */

#define SCAN_BLOCK 256
#define SCAN_ITEMS 16
#define SCAN_TILE (SCAN_BLOCK * SCAN_ITEMS)

DEV uint32_t wave_inclusive_scan(uint32_t v) {
  for (int off = 1; off < WAVE; off <<= 1) {
    uint32_t u = __shfl_up(v, off);
    if ((int)(threadIdx.x & (WAVE - 1)) >= off) v += u;
  }
  return v;
}

/* per-block inclusive scan of a tile; writes tile total to block_sums */
__global__ void k_scan_partial(int64_t n, const uint32_t* in, uint32_t* out,
                               uint32_t* block_sums) {
  __shared__ uint32_t wsum[SCAN_BLOCK / WAVE];
  __shared__ uint32_t carry_s;
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
  int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  uint32_t carry = 0;
  for (int r = 0; r < SCAN_ITEMS; r++) {
    int64_t i = base + r * SCAN_BLOCK + threadIdx.x;
    uint32_t v = (i < n) ? in[i] : 0;
    uint32_t s = wave_inclusive_scan(v);
    if (lane == WAVE - 1) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t acc = 0;
      for (int w = 0; w < SCAN_BLOCK / WAVE; w++) { uint32_t t = wsum[w]; wsum[w] = acc; acc += t; }
      carry_s = acc;
    }
    __syncthreads();
    if (i < n) out[i] = s + wsum[wave] + carry;
    carry += carry_s;
    __syncthreads();
  }
  if (threadIdx.x == 0) block_sums[blockIdx.x] = carry;
}

/* single-block exclusive scan of block_sums (nblocks <= SCAN_TILE * loops) */
__global__ void k_scan_sums(int64_t n, uint32_t* sums) {
  __shared__ uint32_t wsum[SCAN_BLOCK / WAVE];
  __shared__ uint32_t carry_s;
  int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  uint32_t carry = 0;
  for (int64_t base = 0; base < n; base += SCAN_BLOCK) {
    int64_t i = base + threadIdx.x;
    uint32_t v = (i < n) ? sums[i] : 0;
    uint32_t s = wave_inclusive_scan(v);
    if (lane == WAVE - 1) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t acc = 0;
      for (int w = 0; w < SCAN_BLOCK / WAVE; w++) { uint32_t t = wsum[w]; wsum[w] = acc; acc += t; }
      carry_s = acc;
    }
    __syncthreads();
    if (i < n) sums[i] = s - v + wsum[wave] + carry;  /* exclusive */
    carry += carry_s;
    __syncthreads();
  }
}

/* add scanned block sums back; also converts inclusive->exclusive */
__global__ void k_scan_add(int64_t n, const uint32_t* in, uint32_t* out,
                           const uint32_t* block_sums) {
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
  uint32_t add = block_sums[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS; r++) {
    int64_t i = base + r * SCAN_BLOCK + threadIdx.x;
    if (i < n) out[i] = out[i] - in[i] + add;  /* inclusive - v = exclusive */
  }
}

static int exclusive_scan_u32(hipStream_t s, int64_t n, const uint32_t* in,
                              uint32_t* out, uint32_t* block_sums /* >= nblocks+1 */) {
  int64_t nblocks = (n + SCAN_TILE - 1) / SCAN_TILE;
  k_scan_partial<<<dim3((uint32_t)nblocks), SCAN_BLOCK, 0, s>>>(n, in, out, block_sums);
  k_scan_sums<<<1, SCAN_BLOCK, 0, s>>>(nblocks, block_sums);
  k_scan_add<<<dim3((uint32_t)nblocks), SCAN_BLOCK, 0, s>>>(n, in, out, block_sums);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* status word for decoupled lookback: [63:56] epoch, [55:54] status
 * (1 = aggregate, 2 = inclusive prefix), [53:0] value. One 8-byte
 * agent-scope atomic store/load per word (single-granule publish: the
 * payload IS the flag — no fences needed). */
#define OSW_AGG (1ULL << 54)
#define OSW_PFX (2ULL << 54)
#define OSW_VAL(x) ((x) & ((1ULL << 54) - 1))
#define OSW_EPOCH(x) ((x) >> 56)
#define OSW_SPIN_LIMIT (1u << 22)

typedef unsigned long long ull2_a8 __attribute__((vector_size(16), aligned(8)));
typedef uint32_t u32v2_a4 __attribute__((vector_size(8), aligned(4)));

template <int BIN_MODE, int BLOCK, int ITEMS, bool LOOKBACK, typename PayT = uint32_t,
          int RADIX_BITS = 8, bool CONTIG = false>
__global__ __launch_bounds__(BLOCK)
void k_radix_scatter(int64_t n, const uint64_t* kin, const PayT* iin,
                     uint64_t* kout, PayT* iout,
                     const uint32_t* scanned /* [256][nblocks] exclusive */,
                     int shift, int nblocks, int nparts,
                     unsigned long long* state /* [nblocks][256] */,
                     const uint32_t* gbase /* [256] pass bin bases */,
                     unsigned long long* err_flag, uint32_t epoch,
                     void* decode_out /* non-null on the final pass: write
                       decoded keys here instead of encoded keys to kout */,
                     int decode_mode /* 1=i64 2=f64, +4 = desc */,
                     int in_mode /* non-zero on a fused first pass: kin is the
                       caller's raw column (1=i64 2=f64, +4 = desc), encoded
                       in registers; iin == nullptr then means id = row index */) {
  constexpr int WAVES = BLOCK / WAVE;
  constexpr int TILE = BLOCK * ITEMS;
  constexpr int BINS = 1 << RADIX_BITS;
  __shared__ uint32_t wave_hist[WAVES][BINS];
  __shared__ uint32_t bin_start[BINS];    /* in-block exclusive start per bin */
  __shared__ uint32_t bin_gbase[BINS];    /* global dest minus local start    */
  __shared__ uint32_t wtot[WAVES <= 4 ? 4 : WAVES];
  /* narrow-digit cooperative lookback needs each bin's block count visible
   * to its resolver wave */
  __shared__ uint32_t bin_cnt[(LOOKBACK && RADIX_BITS < 8) ? BINS : 1];
  __shared__ uint64_t stage_k[TILE];
  __shared__ PayT stage_i[TILE];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE, lane = tid & (WAVE - 1);
  const int64_t base = (int64_t)blockIdx.x * TILE;
  const int tile_n = (int)min((int64_t)TILE, n - base);

  for (int b = tid; b < WAVES * BINS; b += BLOCK)
    ((uint32_t*)wave_hist)[b] = 0;
  __syncthreads();

  /* wave w owns the contiguous sub-tile [w*WAVE*ITEMS, ...): element order
   * within the block = (wave, round, lane) = linear tile order. */
  uint64_t k[ITEMS];
  PayT id[ITEMS];
  uint16_t lrank[ITEMS];
  uint8_t lbin[ITEMS];

  const int64_t wbase = base + (int64_t)wave * WAVE * ITEMS;
  /* issue every load before the serial ranking chain so all ITEMS pairs
   * are in flight at once (A/B via GPUQ_SCATTER_NO_PRELOAD) */
  if (iin) {
    #pragma unroll
    for (int r = 0; r < ITEMS; r++) {
      int64_t i = wbase + r * WAVE + lane;
      bool valid = i < n;
      k[r] = valid ? kin[i] : 0;
      id[r] = valid ? iin[i] : 0;
    }
  } else {
    /* fused first pass: one 8-byte load per lane (the column may start at
     * any 8-byte offset), the row id is the row's index */
    #pragma unroll
    for (int r = 0; r < ITEMS; r++) {
      int64_t i = wbase + r * WAVE + lane;
      k[r] = i < n ? kin[i] : 0;
      id[r] = (PayT)i;
    }
  }
  if (in_mode) {
    /* rows past n get a meaningless word here; they are never binned or staged */
    #pragma unroll
    for (int r = 0; r < ITEMS; r++) k[r] = sort_in_word(k[r], in_mode);
  }
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    bool valid = i < n;
    int bin = valid ? compute_bin<BIN_MODE>(k[r], shift, nparts) : 0;
    if (RADIX_BITS < 8) bin &= (1 << RADIX_BITS) - 1;
    lbin[r] = (uint8_t)bin;
    /* ballot multi-split: mask of lanes in this wave with the same bin */
    uint64_t active = __ballot(valid);
    uint64_t same = active;
    for (int b = 0; b < RADIX_BITS; b++) {
      uint64_t bl = __ballot((bin >> b) & 1);
      same &= ((bin >> b) & 1) ? bl : ~bl;
    }
    uint64_t below = same & ((1ULL << lane) - 1);
    int rank = __popcll(below);
    int leader = __ffsll((unsigned long long)same) - 1;
    uint32_t basecnt = 0;
    if (valid && lane == leader) {
      basecnt = wave_hist[wave][bin];
      wave_hist[wave][bin] = basecnt + __popcll(same);
    }
    basecnt = __shfl(basecnt, leader);
    lrank[r] = (uint16_t)(basecnt + rank);
    /* wave_hist rows are wave-private: the round-r leader's LDS RMW only
     * needs to be ordered before round r+1's read within THIS wave. DS ops
     * from one wave are serviced in issue order; the wave barrier stops the
     * compiler from reordering them. */
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  /* cross-wave exclusive prefix per bin + block-wide exclusive scan over
   * bins. The first 256 threads each own one bin. */
  uint32_t acc = 0;
  if (tid < BINS) {
    int bin = tid;
    for (int w = 0; w < WAVES; w++) {
      uint32_t t = wave_hist[w][bin];
      wave_hist[w][bin] = acc;
      acc += t;
    }
    if (LOOKBACK) {
      /* publish own AGGREGATE early so successors can proceed */
      __hip_atomic_store(&state[(int64_t)blockIdx.x * 256 + bin],
                         ((unsigned long long)epoch << 56) | OSW_AGG | acc,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (RADIX_BITS < 8) bin_cnt[bin] = acc;
    }
    uint32_t inc = wave_inclusive_scan(acc);
    if (lane == WAVE - 1) wtot[wave] = inc;
    bin_start[bin] = inc - acc;  /* provisional; add wave offsets after sync */
  }
  __syncthreads();
  if (tid < BINS) {
    int bin = tid;
    uint32_t woff = 0;
    for (int w = 0; w < wave; w++) woff += wtot[w];
    uint32_t excl = bin_start[bin] + woff;
    bin_start[bin] = excl;
    if (!LOOKBACK) {
      bin_gbase[bin] = scanned[(int64_t)bin * nblocks + blockIdx.x] - excl;
    } else {
      bin_gbase[bin] = excl;  /* stash; lookback resolves after staging */
    }
  }
  __syncthreads();

  /* stage reordered tile in LDS (lookback waits overlap with this) */
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    if (i < n) {
      uint32_t pos = bin_start[lbin[r]] + wave_hist[wave][lbin[r]] + lrank[r];
      stage_k[pos] = k[r];
      stage_i[pos] = id[r];
    }
  }
  if (LOOKBACK && RADIX_BITS < 8) {
    /* full-wave cooperative lookback: each wave resolves whole bins — all
     * 64 lanes poll one predecessor status word each per round (the
     * per-thread serial walk left only BINS walker lanes active, which
     * measured as the 4-bit mode's wall: 83% WAIT_ANY). Lane j inspects
     * predecessor blockIdx.x-1-j; a ballot finds the newest PREFIX and the
     * first not-ready word, a shuffle reduction sums the consumable run. */
    constexpr int BPW = (BINS + WAVES - 1) / WAVES;
    for (int bi = 0; bi < BPW; bi++) {
      int bin = wave * BPW + bi;
      if (bin >= BINS) break;
      uint32_t excl = bin_gbase[bin];
      unsigned long long pred = 0;
      uint32_t spins = 0;
      int p = (int)blockIdx.x - 1;
      bool failed = false;
      while (p >= 0) {
        int cnt = (p + 1 < WAVE) ? p + 1 : WAVE;
        unsigned long long v = 0;
        bool ready = false, ispfx = false;
        if (lane < cnt) {
          v = __hip_atomic_load(&state[(int64_t)(p - lane) * 256 + bin],
                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ready = OSW_EPOCH(v) == epoch && (v & (OSW_AGG | OSW_PFX));
          ispfx = ready && (v & OSW_PFX);
        }
        uint64_t nr_mask = __ballot(lane < cnt && !ready);
        uint64_t pfx_mask = __ballot(ispfx);
        int first_nr = nr_mask ? __ffsll((unsigned long long)nr_mask) - 1 : 64;
        int first_pfx = pfx_mask ? __ffsll((unsigned long long)pfx_mask) - 1 : 64;
        bool done = first_pfx < first_nr;
        int take = done ? first_pfx + 1 : (first_nr < cnt ? first_nr : cnt);
        if (take == 0) {
          if (++spins > OSW_SPIN_LIMIT) {
            if (lane == 0)
              __hip_atomic_store(err_flag, 1ull, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
            failed = true;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        unsigned long long contrib = (lane < take) ? OSW_VAL(v) : 0;
        #pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1)
          contrib += __shfl_down(contrib, off);
        contrib = __shfl(contrib, 0);
        pred += contrib;
        spins = 0;
        if (done) break;
        p -= take;
      }
      (void)failed;
      if (lane == 0) {
        __hip_atomic_store(&state[(int64_t)blockIdx.x * 256 + bin],
                           ((unsigned long long)epoch << 56) | OSW_PFX |
                               (pred + bin_cnt[bin]),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bin_gbase[bin] = gbase[bin] + (uint32_t)pred - excl;
      }
    }
  } else if (LOOKBACK && tid < 256) {
    int bin = tid;
    uint32_t excl = bin_gbase[bin];
    uint32_t own = acc;   /* this thread's phase-2 block count for its bin */
    /* chunked decoupled lookback: LB predecessor words in flight per step */
    constexpr int LB = 4;
    unsigned long long pred = 0;
    uint32_t spins = 0;
    int p = (int)blockIdx.x - 1;
    while (p >= 0) {
      int cnt = (p + 1 < LB) ? p + 1 : LB;
      unsigned long long v[LB];
      #pragma unroll
      for (int j = 0; j < LB; j++)
        if (j < cnt)
          v[j] = __hip_atomic_load(&state[(int64_t)(p - j) * 256 + bin],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      /* walk newest -> oldest; stop at first PREFIX; retry at not-ready */
      bool stall = false, done = false;
      unsigned long long add = 0;
      #pragma unroll
      for (int j = 0; j < LB; j++) {
        if (j >= cnt || done || stall) continue;
        if (OSW_EPOCH(v[j]) != epoch || !(v[j] & (OSW_AGG | OSW_PFX))) {
          stall = true;
        } else {
          add += OSW_VAL(v[j]);
          if (v[j] & OSW_PFX) done = true;
        }
      }
      if (stall) {
        if (++spins > OSW_SPIN_LIMIT) {        /* bounded: give up, flag host */
          __hip_atomic_store(err_flag, 1ull, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        continue;                               /* retry same chunk */
      }
      pred += add;
      if (done) break;
      p -= cnt;
    }
    /* publish inclusive prefix (even after timeout, to unblock others) */
    __hip_atomic_store(&state[(int64_t)blockIdx.x * 256 + bin],
                       ((unsigned long long)epoch << 56) | OSW_PFX |
                           (pred + own),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bin_gbase[bin] = gbase[bin] + (uint32_t)pred - excl;
  }
  __syncthreads();

  /* drain LDS -> coalesced global runs per bin */
  if (CONTIG) {
    /* contiguous per-thread drain: each thread owns ITEMS consecutive
     * staged elements; same-bin neighbours have consecutive destinations,
     * so pairs collapse into ONE 16 B key store + ONE 8 B id store — the
     * same bytes in HALF the store instructions (the padded-record test
     * showed extra BYTES lose; this halves requests at equal bytes).
     * Needs odd ITEMS for tolerable LDS bank conflicts (stride 2*ITEMS
     * words, gcd 2 -> 2-way). PayT must be 4 B. */
    auto out_word = [&](uint64_t kk) -> uint64_t {
      return sort_out_word(kk, decode_mode);
    };
    uint64_t* kbase = decode_mode ? (uint64_t*)decode_out : kout;
    int j0 = tid * ITEMS;
    int jend = j0 + ITEMS < tile_n ? j0 + ITEMS : tile_n;
    for (int j = j0; j < jend;) {
      uint64_t k0 = stage_k[j];
      int b0 = compute_bin<BIN_MODE>(k0, shift, nparts);
      if (RADIX_BITS < 8) b0 &= (1 << RADIX_BITS) - 1;
      uint32_t dst = bin_gbase[b0] + (uint32_t)j;
      if (j + 1 < jend) {
        uint64_t k1 = stage_k[j + 1];
        int b1 = compute_bin<BIN_MODE>(k1, shift, nparts);
        if (RADIX_BITS < 8) b1 &= (1 << RADIX_BITS) - 1;
        if (b1 == b0) {
          *(ull2_a8*)&kbase[dst] = (ull2_a8){out_word(k0), out_word(k1)};
          *(u32v2_a4*)&iout[dst] =
              (u32v2_a4){(uint32_t)stage_i[j], (uint32_t)stage_i[j + 1]};
          j += 2;
          continue;
        }
      }
      kbase[dst] = out_word(k0);
      iout[dst] = stage_i[j];
      j += 1;
    }
    return;
  }
  for (int r = 0; r < ITEMS; r++) {
    int j = r * BLOCK + tid;
    if (j < tile_n) {
      uint64_t kk = stage_k[j];
      int bin = compute_bin<BIN_MODE>(kk, shift, nparts);
      if (RADIX_BITS < 8) bin &= (1 << RADIX_BITS) - 1;
      uint32_t dst = bin_gbase[bin] + (uint32_t)j;
      /* final pass: emit the DECODED key column directly (the separate
         decode kernel and this pass's encoded-key write both disappear) */
      uint64_t kv_out = sort_out_word(kk, decode_mode);
      void* kdst = decode_mode ? (void*)&((uint64_t*)decode_out)[dst]
                               : (void*)&kout[dst];
#ifdef GPUQ_DRAIN_SC1
      /* write-through: scattered partial-line stores skip the L2
       * write-allocate read-for-ownership (guide: publish-large) */
      __hip_atomic_store((uint64_t*)kdst, kv_out, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store((PayT*)&iout[dst], stage_i[j], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
#elif defined(GPUQ_DRAIN_NT)
      __builtin_nontemporal_store(kv_out, (uint64_t*)kdst);
      __builtin_nontemporal_store(stage_i[j], &iout[dst]);
#else
      *(uint64_t*)kdst = kv_out;
      iout[dst] = stage_i[j];
#endif
    }
  }
}

/* runtime-selectable geometry (GPUQ_SORT_GEOM env: "BLOCKxITEMS") */
static scatter_geom get_sort_geom(void) {
  static scatter_geom g = {0, 0};
  if (g.block == 0) {
    const char* e = getenv("GPUQ_SORT_GEOM");
    int b = 0, it = 0;
    if (e && sscanf(e, "%dx%d", &b, &it) == 2) { g.block = b; g.items = it; }
    else { g.block = 256; g.items = 22; }  /* two-box A/B winner: ~5% over
                                            * 512x10 (fewer waves per
                                            * barrier at the same tile
                                            * residency) */
    /* only geometries with a dispatch entry are legal: an unknown pair
     * would silently run a different tile than the block count assumed
     * (incomplete sort). Clamp to the default. */
    static const int known[][2] = {{256,16},{512,8},{512,16},{1024,8},{512,4},
                                   {512,6},{256,12},{512,12},{1024,5},{512,10},
                                   {1024,2},{1024,6},{1024,4},{512,11},
                                   {256,20},{256,22}};
    bool ok = false;
    for (auto& k : known) ok = ok || (k[0] == g.block && k[1] == g.items);
    if (!ok) {
      fprintf(stderr, "gpuq: unsupported GPUQ_SORT_GEOM %dx%d, using 256x22\n",
              g.block, g.items);
      g.block = 256; g.items = 22;
    }
  }
  return g;
}

template <int BIN_MODE, bool LOOKBACK>
static void launch_scatter(hipStream_t s, scatter_geom g, int64_t nb,
                           int64_t n, const uint64_t* kin, const uint32_t* iin,
                           uint64_t* kout, uint32_t* iout,
                           const uint32_t* scanned, int shift, int nparts,
                           unsigned long long* state, const uint32_t* gbase,
                           unsigned long long* err_flag, uint32_t epoch,
                           void* decode_out = nullptr, int decode_mode = 0,
                           int in_mode = 0) {
  dim3 grid((uint32_t)nb);
#define LS(B, I) k_radix_scatter<BIN_MODE, B, I, LOOKBACK><<<grid, B, 0, s>>>( \
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase, \
      err_flag, epoch, decode_out, decode_mode, in_mode)
  static int contig = -1;
  if (contig < 0) contig = getenv("GPUQ_DRAIN_CONTIG") != nullptr;
  if (contig && g.block == 512 && (g.items == 9 || g.items == 10 || g.items == 11)) {
    if (g.items == 9)
      k_radix_scatter<BIN_MODE, 512, 9, LOOKBACK, uint32_t, 8, true><<<grid, 512, 0, s>>>(
          n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
          err_flag, epoch, decode_out, decode_mode, in_mode);
    else if (g.items == 11)
      k_radix_scatter<BIN_MODE, 512, 11, LOOKBACK, uint32_t, 8, true><<<grid, 512, 0, s>>>(
          n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
          err_flag, epoch, decode_out, decode_mode, in_mode);
    else
      k_radix_scatter<BIN_MODE, 512, 10, LOOKBACK, uint32_t, 8, true><<<grid, 512, 0, s>>>(
          n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
          err_flag, epoch, decode_out, decode_mode, in_mode);
    return;
  }
  if (g.block == 256 && g.items == 20)
    k_radix_scatter<BIN_MODE, 256, 20, LOOKBACK><<<grid, 256, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 256 && g.items == 22)
    k_radix_scatter<BIN_MODE, 256, 22, LOOKBACK><<<grid, 256, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 512 && g.items == 11)
    k_radix_scatter<BIN_MODE, 512, 11, LOOKBACK><<<grid, 512, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 256 && g.items == 16) LS(256, 16);
  else if (g.block == 512 && g.items == 8) LS(512, 8);
  else if (g.block == 512 && g.items == 16) LS(512, 16);
  else if (g.block == 1024 && g.items == 8) LS(1024, 8);
  else if (g.block == 512 && g.items == 4) LS(512, 4);
  else if (g.block == 512 && g.items == 6)
    k_radix_scatter<BIN_MODE, 512, 6, LOOKBACK><<<grid, 512, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 256 && g.items == 12)
    k_radix_scatter<BIN_MODE, 256, 12, LOOKBACK><<<grid, 256, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 512 && g.items == 12)
    k_radix_scatter<BIN_MODE, 512, 12, LOOKBACK><<<grid, 512, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 1024 && g.items == 5)
    k_radix_scatter<BIN_MODE, 1024, 5, LOOKBACK><<<grid, 1024, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 512 && g.items == 10)
    k_radix_scatter<BIN_MODE, 512, 10, LOOKBACK><<<grid, 512, 0, s>>>(
      n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
      err_flag, epoch, decode_out, decode_mode, in_mode);
  else if (g.block == 1024 && g.items == 2) LS(1024, 2);
  else if (g.block == 1024 && g.items == 6) LS(1024, 6);
  else LS(1024, 4);
#undef LS
}

/* ---- scatter phase ablation (diagnostic only; tools/diag_scatter.py) ----
 * MODE 0: loads only (checksummed against DCE)  1: +ranking  2: +staging
 * 3: +drain (= the real kernel's work). Geometry fixed 512x10. */
template <int MODE>
__global__ __launch_bounds__(512)
void k_scatter_ablate(int64_t n, const uint64_t* kin, const uint32_t* iin,
                      uint64_t* kout, uint32_t* iout,
                      const uint32_t* gbase, unsigned long long* sink,
                      int shift) {
  constexpr int BLOCK = 512, ITEMS = 10, WAVES = BLOCK / WAVE;
  constexpr int TILE = BLOCK * ITEMS;
  __shared__ uint32_t wave_hist[WAVES][256];
  __shared__ uint32_t bin_start[256];
  __shared__ uint32_t bin_gbase[256];
  __shared__ uint32_t wtot[WAVES < 4 ? 4 : WAVES];
  __shared__ uint64_t stage_k[TILE];
  __shared__ uint32_t stage_i[TILE];
  const int tid = threadIdx.x;
  const int wave = tid / WAVE, lane = tid & (WAVE - 1);
  const int64_t base = (int64_t)blockIdx.x * TILE;
  const int tile_n = (int)min((int64_t)TILE, n - base);
  for (int b = tid; b < WAVES * 256; b += BLOCK) ((uint32_t*)wave_hist)[b] = 0;
  __syncthreads();
  uint64_t k[ITEMS]; uint32_t id[ITEMS]; uint16_t lrank[ITEMS]; uint8_t lbin[ITEMS];
  const int64_t wbase = base + (int64_t)wave * WAVE * ITEMS;
  #pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    bool valid = i < n;
    k[r] = valid ? kin[i] : 0;
    id[r] = valid ? iin[i] : 0;
  }
  if (MODE == 0) {
    uint64_t acc = 0;
    for (int r = 0; r < ITEMS; r++) acc ^= k[r] + id[r];
    if (acc == 0xDEADBEEFCAFEBABEull) atomicAdd(sink, 1ull);  /* keep loads */
    return;
  }
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    bool valid = i < n;
    int bin = valid ? (int)((k[r] >> shift) & 0xff) : 0;
    lbin[r] = (uint8_t)bin;
    uint64_t m = __ballot(valid);
    for (int b = 0; b < 8; b++) {
      uint64_t bl = __ballot((bin >> b) & 1);
      m &= ((bin >> b) & 1) ? bl : ~bl;
    }
    uint64_t below = m & ((1ULL << lane) - 1);
    int rank = __popcll(below);
    int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t basecnt = 0;
    if (valid && lane == leader) {
      basecnt = wave_hist[wave][bin];
      wave_hist[wave][bin] = basecnt + __popcll(m);
    }
    basecnt = __shfl(basecnt, leader);
    lrank[r] = (uint16_t)(basecnt + rank);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  uint32_t acc = 0;
  if (tid < 256) {
    int bin = tid;
    for (int w = 0; w < WAVES; w++) {
      uint32_t t = wave_hist[w][bin];
      wave_hist[w][bin] = acc; acc += t;
    }
    uint32_t inc = wave_inclusive_scan(acc);
    if (lane == WAVE - 1) wtot[wave] = inc;
    bin_start[bin] = inc - acc;
  }
  __syncthreads();
  if (tid < 256) {
    int bin = tid;
    uint32_t woff = 0;
    for (int w = 0; w < wave; w++) woff += wtot[w];
    uint32_t excl = bin_start[bin] + woff;
    bin_start[bin] = excl;
    /* realistic layout: uniform data contributes ~TILE/256 rows per bin per
     * block, so block b's bin-k run starts near gbase[k] + b*TILE/256 —
     * the same write pattern the real scanned offsets produce */
    bin_gbase[bin] = gbase[bin] + (uint32_t)(base >> 8) - excl;
  }
  __syncthreads();
  if (MODE == 1) {
    uint32_t a2 = 0;
    for (int r = 0; r < ITEMS; r++) a2 += lrank[r] + bin_start[lbin[r]];
    if (a2 == 0xDEADBEEFu) atomicAdd(sink, 1ull);
    return;
  }
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    if (i < n) {
      uint32_t pos = bin_start[lbin[r]] + wave_hist[wave][lbin[r]] + lrank[r];
      stage_k[pos] = k[r];
      stage_i[pos] = id[r];
    }
  }
  __syncthreads();
  if (MODE == 2) {
    uint64_t a3 = stage_k[tid] + stage_i[TILE - 1 - tid];
    if (a3 == 0xDEADBEEFCAFEBABEull) atomicAdd(sink, 1ull);
    return;
  }
  for (int r = 0; r < ITEMS; r++) {
    int j = r * BLOCK + tid;
    if (j < tile_n) {
      uint64_t kk = stage_k[j];
      int bin = (int)((kk >> shift) & 0xff);
      uint32_t dst = (bin_gbase[bin] + (uint32_t)j) % (uint32_t)n;
      kout[dst] = kk;
      iout[dst] = stage_i[j];
    }
  }
}

/* MODE 4/5: 512x8 tile-4096 variant comparing drain store shapes:
 * 4 = two stores per element (8B key + 4B idx, separate arrays, as shipped)
 * 5 = one 16B record store per element (key, idx, pad) */
template <int MODE>
__global__ __launch_bounds__(512)
void k_scatter_ablate2(int64_t n, const uint64_t* kin, const uint32_t* iin,
                       uint64_t* kout, uint32_t* iout, uint32_t* rout,
                       const uint32_t* gbase, int shift) {
  constexpr int BLOCK = 512, ITEMS = 8;
  constexpr int WAVES = BLOCK / WAVE;
  constexpr int TILE = BLOCK * ITEMS;
  __shared__ uint32_t wave_hist[WAVES][256];
  __shared__ uint32_t bin_start[256];
  __shared__ uint32_t bin_gbase[256];
  __shared__ uint32_t wtot[WAVES];
  __shared__ uint64_t stage_k[TILE];
  __shared__ uint32_t stage_i[TILE];
  const int tid = threadIdx.x;
  const int wave = tid / WAVE, lane = tid & (WAVE - 1);
  const int64_t base = (int64_t)blockIdx.x * TILE;
  const int tile_n = (int)min((int64_t)TILE, n - base);
  for (int b = tid; b < WAVES * 256; b += BLOCK) ((uint32_t*)wave_hist)[b] = 0;
  __syncthreads();
  uint64_t k[ITEMS]; uint32_t id[ITEMS]; uint16_t lrank[ITEMS]; uint8_t lbin[ITEMS];
  const int64_t wbase = base + (int64_t)wave * WAVE * ITEMS;
  #pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    bool valid = i < n;
    k[r] = valid ? kin[i] : 0;
    id[r] = valid ? iin[i] : 0;
  }
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    bool valid = i < n;
    int bin = valid ? (int)((k[r] >> shift) & 0xff) : 0;
    lbin[r] = (uint8_t)bin;
    uint64_t m = __ballot(valid);
    for (int b = 0; b < 8; b++) {
      uint64_t bl = __ballot((bin >> b) & 1);
      m &= ((bin >> b) & 1) ? bl : ~bl;
    }
    uint64_t below = m & ((1ULL << lane) - 1);
    int rank = __popcll(below);
    int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t basecnt = 0;
    if (valid && lane == leader) {
      basecnt = wave_hist[wave][bin];
      wave_hist[wave][bin] = basecnt + __popcll(m);
    }
    basecnt = __shfl(basecnt, leader);
    lrank[r] = (uint16_t)(basecnt + rank);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  if (tid < 256) {
    int bin = tid;
    uint32_t acc = 0;
    for (int w = 0; w < WAVES; w++) {
      uint32_t t = wave_hist[w][bin];
      wave_hist[w][bin] = acc; acc += t;
    }
    uint32_t inc = wave_inclusive_scan(acc);
    if (lane == WAVE - 1) wtot[wave] = inc;
    bin_start[bin] = inc - acc;
  }
  __syncthreads();
  if (tid < 256) {
    int bin = tid;
    uint32_t woff = 0;
    for (int w = 0; w < wave; w++) woff += wtot[w];
    uint32_t excl = bin_start[bin] + woff;
    bin_start[bin] = excl;
    bin_gbase[bin] = gbase[bin] + (uint32_t)(base >> 8) - excl;
  }
  __syncthreads();
  for (int r = 0; r < ITEMS; r++) {
    int64_t i = wbase + r * WAVE + lane;
    if (i < n) {
      uint32_t pos = bin_start[lbin[r]] + wave_hist[wave][lbin[r]] + lrank[r];
      stage_k[pos] = k[r];
      stage_i[pos] = id[r];
    }
  }
  __syncthreads();
  for (int r = 0; r < ITEMS; r++) {
    int j = r * BLOCK + tid;
    if (j < tile_n) {
      uint64_t kk = stage_k[j];
      int bin = (int)((kk >> shift) & 0xff);
      uint32_t dst = (bin_gbase[bin] + (uint32_t)j) % (uint32_t)n;
      if (MODE == 4) {
        kout[dst] = kk;
        iout[dst] = stage_i[j];
      } else {
        uint4 rec;
        rec.x = (uint32_t)kk; rec.y = (uint32_t)(kk >> 32);
        rec.z = stage_i[j]; rec.w = 0;
        ((uint4*)rout)[dst] = rec;
      }
    }
  }
}

extern "C" int gpuq_scatter_ablate2(void* stream, int64_t n, const void* kin,
                                    const void* iin, void* kout, void* iout,
                                    void* rout, const void* gbase, int32_t mode) {
  hipStream_t s = (hipStream_t)stream;
  int64_t nb = (n + 4095) / 4096;
  if (mode == 4)
    k_scatter_ablate2<4><<<dim3((uint32_t)nb), 512, 0, s>>>(
        n, (const uint64_t*)kin, (const uint32_t*)iin, (uint64_t*)kout,
        (uint32_t*)iout, (uint32_t*)rout, (const uint32_t*)gbase, 0);
  else
    k_scatter_ablate2<5><<<dim3((uint32_t)nb), 512, 0, s>>>(
        n, (const uint64_t*)kin, (const uint32_t*)iin, (uint64_t*)kout,
        (uint32_t*)iout, (uint32_t*)rout, (const uint32_t*)gbase, 0);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

extern "C" int gpuq_scatter_ablate(void* stream, int64_t n, const void* kin,
                                   const void* iin, void* kout, void* iout,
                                   const void* gbase, void* sink, int32_t mode) {
  hipStream_t s = (hipStream_t)stream;
  int64_t nb = (n + 5119) / 5120;
  dim3 g((uint32_t)nb);
#define AB(M) k_scatter_ablate<M><<<g, 512, 0, s>>>(n, (const uint64_t*)kin, \
    (const uint32_t*)iin, (uint64_t*)kout, (uint32_t*)iout, \
    (const uint32_t*)gbase, (unsigned long long*)sink, 0)
  if (mode == 0) AB(0); else if (mode == 1) AB(1);
  else if (mode == 2) AB(2); else AB(3);
#undef AB
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

template <int BIN_MODE, bool LOOKBACK>
static void launch_scatter4(hipStream_t s, scatter_geom g, int64_t nb,
                            int64_t n, const uint64_t* kin, const uint32_t* iin,
                            uint64_t* kout, uint32_t* iout,
                            const uint32_t* scanned, int shift, int nparts,
                            unsigned long long* state, const uint32_t* gbase,
                            unsigned long long* err_flag, uint32_t epoch,
                            void* decode_out = nullptr, int decode_mode = 0) {
  dim3 grid((uint32_t)nb);
  if (g.block == 1024 && g.items == 8)
    k_radix_scatter<BIN_MODE, 1024, 8, LOOKBACK, uint32_t, 4><<<grid, 1024, 0, s>>>(
        n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
        err_flag, epoch, decode_out, decode_mode, 0 /* in_mode: never fused */);
  else if (g.block == 256 && g.items == 22)
    k_radix_scatter<BIN_MODE, 256, 22, LOOKBACK, uint32_t, 4><<<grid, 256, 0, s>>>(
        n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
        err_flag, epoch, decode_out, decode_mode, 0 /* in_mode: never fused */);
  else if (g.block == 512 && g.items == 10)
    k_radix_scatter<BIN_MODE, 512, 10, LOOKBACK, uint32_t, 4><<<grid, 512, 0, s>>>(
        n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
        err_flag, epoch, decode_out, decode_mode, 0 /* in_mode: never fused */);
  else
    k_radix_scatter<BIN_MODE, 512, 10, LOOKBACK, uint32_t, 4><<<grid, 512, 0, s>>>(
        n, kin, iin, kout, iout, scanned, shift, (int)nb, nparts, state, gbase,
        err_flag, epoch, decode_out, decode_mode, 0 /* in_mode: never fused */);  /* unreachable: gated above */
}

/* decode sorted keys back to the output dtype */
template <int DTYPE, bool DESC>
__global__ void k_decode(int64_t n, const uint64_t* ek, void* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t e = ek[i];
    if (DESC) e = ~e;
    if (DTYPE == GPUQ_FLOAT64) {
      uint64_t mask = ((e >> 63) ? 0 : ~0ULL) | SIGNBIT;  /* inverse bijection */
      ((uint64_t*)out)[i] = e ^ mask;
    } else {
      ((int64_t*)out)[i] = (int64_t)(e ^ SIGNBIT);
    }
  }
}

/* ---- prefix plan: tie-fix after the leading-window passes ----
 * Input: (encoded key, rowid) pairs stably ordered by `key >> shift` (the
 * leading window; bytes above `shift` outside it are constant). A run is a
 * maximal stretch of equal `key >> shift`. Runs of up to GPUQ_SORT_TIE_MAX
 * rows are ranked by (key, position) — inside a run that is the order of the
 * deferred low bits, ties in input order — and written to run_start + rank.
 * Longer runs are written in place: fully-equal keys are already in stable
 * order; a descent inside one raises *overflow and the host redoes the sort
 * with the full pass list. Runs cross tile edges, so each block stages its
 * tile with a GPUQ_SORT_TIE_MAX-row halo on both sides. */
#define GPUQ_SORT_TIE_MAX 32
#define TIEFIX_BLOCK 256
#define TIEFIX_ITEMS 8
#define TIEFIX_TILE (TIEFIX_BLOCK * TIEFIX_ITEMS) /* 2048 */

__global__ __launch_bounds__(TIEFIX_BLOCK)
void k_sort_tiefix(int64_t n, const uint64_t* kin, const uint32_t* iin,
                   uint32_t* out_perm, uint64_t* out_keys /* may be null */,
                   int shift, int decode_mode, unsigned long long* overflow) {
  constexpr int HALO = GPUQ_SORT_TIE_MAX;
  __shared__ uint64_t tk[TIEFIX_TILE + 2 * HALO];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * TIEFIX_TILE;
  uint32_t id[TIEFIX_ITEMS];
  #pragma unroll
  for (int r = 0; r < TIEFIX_ITEMS; r++) {
    int64_t i = base + r * TIEFIX_BLOCK + tid;
    id[r] = i < n ? iin[i] : 0;
  }
  for (int j = tid; j < TIEFIX_TILE + 2 * HALO; j += TIEFIX_BLOCK) {
    int64_t g = base - HALO + j;
    tk[j] = (g >= 0 && g < n) ? kin[g] : 0;
  }
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < TIEFIX_ITEMS; r++) {
    const int j = r * TIEFIX_BLOCK + tid;
    const int64_t i = base + j;
    if (i >= n) break;
    const uint64_t* c = &tk[HALO + j];   /* c[t] = key of row i+t, |t| <= HALO */
    const uint64_t k = c[0];
    const uint64_t win = k >> shift;
    /* bounds come from the row index, never from the staged zero fill */
    int back = 0, fwd = 0;
    while (back < HALO && i - back - 1 >= 0 && (c[-back - 1] >> shift) == win) back++;
    while (fwd < HALO && i + fwd + 1 < n && (c[fwd + 1] >> shift) == win) fwd++;
    int64_t dst = i;
    if (back + fwd) {
      if (back + fwd + 1 <= GPUQ_SORT_TIE_MAX) {
        /* neither scan hit its cap: [i-back, i+fwd] is the whole run */
        int rank = 0;
        for (int t = -back; t <= fwd; t++) {
          uint64_t o = c[t];
          rank += (o < k) || (o == k && t < 0);
        }
        dst = i - back + rank;
      } else if (back > 0 && c[-1] > k) {
        __hip_atomic_store(overflow, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    out_perm[dst] = id[r];
    if (out_keys) out_keys[dst] = sort_out_word(k, decode_mode);
  }
}

/* prefix-plan rule (host): the leading window is the top H active bytes, H
 * the smallest count whose changed bits reach ceil(log2(n)) + 2; the lower
 * active bytes are deferred to the tie-fix. Taken only when at least
 * SORT_PREFIX_MIN_DEFERRED bytes are deferred and the expected number of
 * same-window partners per row, n * prod_{window bytes} sum_v p_v^2 (byte
 * independence), is at most 1. Returns the lowest window byte, or -1. */
#define SORT_PREFIX_MIN_DEFERRED 2
static int sort_prefix_plan(uint64_t bits_changed, const uint32_t* hghist /* [8][256] */,
                            int64_t n, int* window_passes, int* deferred_bytes) {
  int need = 2;
  while (((int64_t)1 << (need - 2)) < n) need++;
  int bits = 0, npass = 0, low = -1;
  for (int b = 7; b >= 0 && bits < need; b--) {
    unsigned ch = (unsigned)((bits_changed >> (b * 8)) & 0xff);
    if (!ch) continue;
    bits += __builtin_popcount(ch);
    npass++;
    low = b;
  }
  if (bits < need) return -1;
  int deferred = 0;
  for (int b = 0; b < low; b++)
    if ((bits_changed >> (b * 8)) & 0xff) deferred++;
  if (deferred < SORT_PREFIX_MIN_DEFERRED) return -1;
  double est = (double)n;
  for (int b = low; b < 8; b++) {
    if (!((bits_changed >> (b * 8)) & 0xff)) continue;
    double s = 0.0;
    for (int v = 0; v < 256; v++) {
      double p = (double)hghist[b * 256 + v] / (double)n;
      s += p * p;
    }
    est *= s;
  }
  if (est > 1.0) return -1;
  *window_passes = npass;
  *deferred_bytes = deferred;
  return low;
}

struct sort_plan_rec { int window_passes, deferred_bytes, fell_back; };
static __thread sort_plan_rec g_sort_plan;

extern "C" void gpuq_sort_last_plan(int* window_passes, int* deferred_bytes,
                                    int* fell_back) {
  if (window_passes) *window_passes = g_sort_plan.window_passes;
  if (deferred_bytes) *deferred_bytes = g_sort_plan.deferred_bytes;
  if (fell_back) *fell_back = g_sort_plan.fell_back;
}

/* workspace layout for sort/partition (geometry-aware: the GPUQ_SORT_GEOM
 * env must not change between workspace sizing and the sort call) */
struct sort_ws {
  uint64_t* ka; uint64_t* kb;
  uint32_t* ia; uint32_t* ib;
  uint32_t* hist; uint32_t* hist_scan; uint32_t* block_sums;
  unsigned long long* bits; /* [0]=and [1]=or */
  uint32_t* ghist;          /* [8][256] global byte histograms */
  uint32_t* gbase;          /* [8][256] per-pass exclusive bin bases */
  unsigned long long* state; /* [nblocks][256] lookback status words */
  unsigned long long* err;   /* [0] lookback timeout flag, [1] tie-fix overflow */
};

static int64_t sort_nblocks(int64_t n, int tile) { return (n + tile - 1) / tile; }

static void sort_ws_layout(int64_t n, int nbins, sort_ws* w, char* basep, int64_t* total) {
  int tile = get_sort_geom().block * get_sort_geom().items;
  int64_t nb = sort_nblocks(n, tile);
  int64_t hist_n = (int64_t)nbins * nb;
  int64_t scan_blocks = (hist_n + SCAN_TILE - 1) / SCAN_TILE + 1;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = basep ? basep + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->ka = (uint64_t*)take(n * 8);
  w->kb = (uint64_t*)take(n * 8);
  w->ia = (uint32_t*)take(n * 4);
  w->ib = (uint32_t*)take(n * 4);
  w->hist = (uint32_t*)take(hist_n * 4);
  w->hist_scan = (uint32_t*)take(hist_n * 4);
  w->block_sums = (uint32_t*)take(scan_blocks * 4);
  w->bits = (unsigned long long*)take(16);
  w->ghist = (uint32_t*)take(8 * 256 * 4);
  w->gbase = (uint32_t*)take(8 * 256 * 4);
  w->state = (unsigned long long*)take(nb * 256 * 8);
  w->err = (unsigned long long*)take(16);  /* [0] lookback timeout, [1] tie-fix overflow */
  *total = off;
}

extern "C" int64_t gpuq_sort_workspace_bytes(int64_t n) {
  sort_ws w; int64_t total;
  sort_ws_layout(n, 256, &w, nullptr, &total);
  return total;
}

/* hist_only: the pre-pass of the fused first scatter pass — reduction and
 * histograms only, w->ka / w->ia stay unwritten (no rowmap in that mode) */
static void launch_encode(hipStream_t s, int64_t n, const void* keys,
                          const uint32_t* rowmap, int dtype, int desc, sort_ws* w,
                          bool hist_only = false) {
  uint64_t* ek = hist_only ? nullptr : w->ka;
  uint32_t* idx = hist_only ? nullptr : w->ia;
  if (dtype == GPUQ_FLOAT64) {
    if (desc) k_encode<GPUQ_FLOAT64, true><<<grid1d(n), 256, 0, s>>>(n, keys, rowmap, ek, idx, &w->bits[0], &w->bits[1], w->ghist);
    else      k_encode<GPUQ_FLOAT64, false><<<grid1d(n), 256, 0, s>>>(n, keys, rowmap, ek, idx, &w->bits[0], &w->bits[1], w->ghist);
  } else {
    if (desc) k_encode<GPUQ_INT64, true><<<grid1d(n), 256, 0, s>>>(n, keys, rowmap, ek, idx, &w->bits[0], &w->bits[1], w->ghist);
    else      k_encode<GPUQ_INT64, false><<<grid1d(n), 256, 0, s>>>(n, keys, rowmap, ek, idx, &w->bits[0], &w->bits[1], w->ghist);
  }
}

extern "C" int gpuq_sort_perm(void* stream, int64_t n, gpuq_col key,
                              int32_t desc, int32_t nulls_first,
                              uint32_t* out_perm, void* out_keys,
                              void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n > 0xFFFFFFFFLL) FAIL(GPUQ_ERR_INVALID, "sort: nrows %lld > 2^32", (long long)n);
  if (key.dtype != GPUQ_INT64 && key.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "sort: unsupported dtype %d", key.dtype);
  sort_ws w; int64_t need;
  sort_ws_layout(n, 256, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "sort: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
  if (n == 0) return GPUQ_OK;

  scatter_geom geom = get_sort_geom();
  int tile = geom.block * geom.items;
  static __thread int force_classic = 0;
  static __thread int force_no_prefix = 0;
  bool onesweep = !force_classic && getenv("GPUQ_NO_ONESWEEP") == nullptr;
  bool no_prefix = force_no_prefix || getenv("GPUQ_SORT_NO_PREFIX") != nullptr;
  g_sort_plan = sort_plan_rec{0, 0, 0};

  /* NULL keys: stable split into [nulls][valids] (or the reverse) per
   * nullOrdering (SortOrder.scala:35-45), then radix-sort the valid subset
   * through a row map; the final permutation is the concatenation. */
  int64_t n_sort = n;           /* rows entering the radix passes */
  int64_t sorted_at = 0;        /* offset of the sorted segment in out_perm */
  const uint32_t* rowmap = nullptr;
  if (key.validity) {
    int64_t nbv = sort_nblocks(n, tile);
    HIP_TRY(hipMemsetAsync(w.err, 0, 8, s));
    k_validity_pids<<<grid1d(n), 256, 0, s>>>(n, key.validity, nulls_first,
                                              w.ka, w.ia, w.err);
    HIP_TRY(hipGetLastError());
    k_radix_hist<0><<<dim3((uint32_t)nbv), 256, 0, s>>>(n, w.ka, 0, w.hist, (int)nbv, tile);
    HIP_TRY(hipGetLastError());
    int rc = exclusive_scan_u32(s, 256 * nbv, w.hist, w.hist_scan, w.block_sums);
    if (rc) return rc;
    launch_scatter<0, false>(s, geom, nbv, n, w.ka, w.ia, w.kb, w.ib, w.hist_scan,
                             0, 0, nullptr, nullptr, nullptr, 0);
    HIP_TRY(hipGetLastError());
    unsigned long long hnull = 0;
    HIP_TRY(hipMemcpyAsync(&hnull, w.err, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int64_t nnull = (int64_t)hnull;
    n_sort = n - nnull;
    sorted_at = nulls_first ? nnull : 0;
    int64_t nulls_at_out = nulls_first ? 0 : n_sort;      /* in out_perm */
    int64_t nulls_at_ib = nulls_first ? 0 : n_sort;       /* in w.ib (same order) */
    if (nnull > 0)
      HIP_TRY(hipMemcpyAsync(out_perm + nulls_at_out, w.ib + nulls_at_ib,
                             nnull * 4, hipMemcpyDeviceToDevice, s));
    rowmap = w.ib + sorted_at;   /* valid rows, input order; consumed by encode */
    if (n_sort == 0) {
      if (out_keys) {
        gpuq_col kc = key; kc.validity = nullptr;
        return gpuq_gather(stream, n, kc, out_perm, out_keys);
      }
      return GPUQ_OK;
    }
  }

  int64_t nb = sort_nblocks(n_sort, tile);
  HIP_TRY(hipMemsetAsync(w.bits, 0, 16, s));
  HIP_TRY(hipMemsetAsync(w.bits, 0xFF, 8, s));  /* bits_and = ~0 */
  HIP_TRY(hipMemsetAsync(w.ghist, 0, 8 * 256 * 4, s));
  bool nibble_mode = onesweep && getenv("GPUQ_SORT_BITS") != nullptr &&
                     atoi(getenv("GPUQ_SORT_BITS")) == 4;
  /* the 4-bit kernel templates exist for these geometries only; a tile
   * mismatch would overlap blocks (wrong results) — fall back to 8-bit */
  if (nibble_mode && !((geom.block == 1024 && geom.items == 8) ||
                       (geom.block == 512 && geom.items == 10) ||
                       (geom.block == 256 && geom.items == 22)))
    nibble_mode = false;
  /* fused first pass: the first scatter pass reads the caller's column and
   * encodes in registers, so only the reduction and the histograms are
   * needed up front (k_encode in histogram-only mode). The column is then
   * read again by that pass and by a redo, and the final pass may write
   * out_keys while the column is still being read: an out_keys that overlaps
   * it takes the materialising path. */
  const char* kraw = (const char*)key.data;
  bool keys_alias = out_keys && (const char*)out_keys < kraw + n * 8 &&
                    kraw < (const char*)out_keys + n * 8;
  bool fused = onesweep && !nibble_mode && !key.validity && !keys_alias &&
               getenv("GPUQ_SORT_NO_FUSED_ENCODE") == nullptr;
  const int key_mode = (key.dtype == GPUQ_FLOAT64 ? 2 : 1) | (desc ? 4 : 0);
  /* encode + skip-byte reduction + all-byte global histograms (one read) */
  { hipEvent_t _pe = prof_begin(s);
  launch_encode(s, n_sort, key.data, rowmap, key.dtype, desc, &w, fused);
  prof_end(fused ? "sort_hist" : "encode", s, _pe); }
  HIP_TRY(hipGetLastError());
  unsigned long long hb[2];
  uint32_t hghist[8 * 256];
  HIP_TRY(hipMemcpyAsync(hb, w.bits, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hghist, w.ghist, sizeof(hghist), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  uint64_t bits_changed = hb[0] ^ hb[1];
  if (fused && bits_changed == 0) {
    /* all keys equal: no pass runs, and the zero-pass tail below copies the
     * identity row ids and decodes the keys from w.ia / w.ka — materialise
     * them. (The device-side ghist counts twice after this; only the host
     * copy above is used from here on.) */
    fused = false;
    { hipEvent_t _pe = prof_begin(s);
    launch_encode(s, n_sort, key.data, nullptr, key.dtype, desc, &w);
    prof_end("encode", s, _pe); }
    HIP_TRY(hipGetLastError());
  }
  int retries = 0;
retry:
  /* prefix plan: radix only the leading window, fix ties in one pass */
  int prefix_low = -1;
  if (!nibble_mode && !no_prefix) {
    int wp = 0, db = 0;
    prefix_low = sort_prefix_plan(bits_changed, hghist, n_sort, &wp, &db);
    if (prefix_low >= 0) g_sort_plan = sort_plan_rec{wp, db, 0};
  }
  if (onesweep && !nibble_mode) {
    /* per-pass exclusive bin bases from the one-read global histograms
     * (replaces the per-pass hist kernel + device scan) */
    uint32_t hgbase[8 * 256];
    for (int b = 0; b < 8; b++) {
      uint32_t run = 0;
      for (int bin = 0; bin < 256; bin++) {
        hgbase[b * 256 + bin] = run;
        run += hghist[b * 256 + bin];
      }
    }
    HIP_TRY(hipMemcpyAsync(w.gbase, hgbase, sizeof(hgbase), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(w.state, 0, nb * 256 * 8, s));
    HIP_TRY(hipMemsetAsync(w.err, 0, 16, s));
  } else if (nibble_mode) {
    /* 16 levels of 4-bit digits (16-bin drains write 16x-longer runs);
     * level bases derived from the same byte histograms */
    uint32_t hgbase[16 * 16];
    for (int lvl = 0; lvl < 16; lvl++) {
      int byte = lvl / 2;
      bool high = lvl & 1;
      uint32_t cnt[16] = {0};
      for (int v = 0; v < 256; v++) {
        int nib = high ? (v >> 4) : (v & 15);
        cnt[nib] += hghist[byte * 256 + v];
      }
      uint32_t run = 0;
      for (int v = 0; v < 16; v++) { hgbase[lvl * 16 + v] = run; run += cnt[v]; }
    }
    HIP_TRY(hipMemcpyAsync(w.gbase, hgbase, sizeof(hgbase), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(w.state, 0, nb * 256 * 8, s));
    HIP_TRY(hipMemsetAsync(w.err, 0, 16, s));
  } else if (prefix_low >= 0) {
    HIP_TRY(hipMemsetAsync(w.err, 0, 16, s));
  }

  /* last active pass writes row ids straight into out_perm (saves the
   * 4 B/row device copy) */
  int nlevels = nibble_mode ? 16 : 8;
  int lvl_bits = nibble_mode ? 4 : 8;
  uint64_t lvl_mask = nibble_mode ? 0xfULL : 0xffULL;
  int last_byte = -1;
  for (int lvl = 0; lvl < nlevels; lvl++)
    if (((bits_changed >> (lvl * lvl_bits)) & lvl_mask) != 0) last_byte = lvl;
  /* pass input: the ping-pong scratch, or on the fused first pass the
   * caller's column (read-only: it never enters kout/knext, the two buffers
   * the passes write) with row ids synthesised from the row index */
  const uint64_t* kin = fused ? (const uint64_t*)key.data : w.ka;
  const uint32_t* iin = fused ? nullptr : w.ia;
  uint64_t *kout = w.kb, *knext = w.ka;
  uint32_t *iout = w.ib, *inext = w.ia;
  int in_mode = fused ? key_mode : 0;   /* cleared after the first active pass */
  for (int byte = 0; byte < nlevels; byte++) {
    if (((bits_changed >> (byte * lvl_bits)) & lvl_mask) == 0) continue;  /* RadixSort.java:126 skip */
    if (byte < prefix_low) continue;  /* deferred to the tie-fix */
    int shift = byte * lvl_bits;
    /* under the prefix plan every pass stays in the ping-pong buffers; the
     * tie-fix writes out_perm and the decoded keys */
    bool final_pass = byte == last_byte && prefix_low < 0;
    uint32_t* iout_pass = final_pass ? out_perm + sorted_at : iout;
    /* fuse the key decode into the final pass when the caller wants keys
     * and the null path is not rerouting them through a gather */
    void* dec_out = nullptr;
    int dec_mode = 0;
    if (final_pass && out_keys && !key.validity) {
      dec_out = (char*)out_keys;  /* sorted_at == 0 without validity */
      dec_mode = (key.dtype == GPUQ_FLOAT64 ? 2 : 1) | (desc ? 4 : 0);
    }
    if (nibble_mode) {
      { hipEvent_t _pe = prof_begin(s);
      launch_scatter4<0, true>(s, geom, nb, n_sort, kin, iin, kout, iout_pass, nullptr,
                               shift, 0, w.state, w.gbase + byte * 16, w.err,
                               (uint32_t)(byte + 1), dec_out, dec_mode);
      prof_end("radix_scatter", s, _pe); }
      HIP_TRY(hipGetLastError());
    } else if (onesweep) {
      { hipEvent_t _pe = prof_begin(s);
      launch_scatter<0, true>(s, geom, nb, n_sort, kin, iin, kout, iout_pass, nullptr,
                              shift, 0, w.state, w.gbase + byte * 256, w.err,
                              (uint32_t)(byte + 1), dec_out, dec_mode, in_mode);
      prof_end("radix_scatter", s, _pe); }
      HIP_TRY(hipGetLastError());
    } else {
      { hipEvent_t _pe = prof_begin(s);
      k_radix_hist<0><<<dim3((uint32_t)nb), 256, 0, s>>>(n_sort, kin, shift, w.hist, (int)nb, tile);
      prof_end("radix_hist", s, _pe); }
      HIP_TRY(hipGetLastError());
      int rc = exclusive_scan_u32(s, (int64_t)256 * nb, w.hist, w.hist_scan, w.block_sums);
      if (rc) return rc;
      { hipEvent_t _pe = prof_begin(s);
      launch_scatter<0, false>(s, geom, nb, n_sort, kin, iin, kout, iout_pass, w.hist_scan,
                               shift, 0, nullptr, nullptr, nullptr, 0, dec_out, dec_mode);
      prof_end("radix_scatter", s, _pe); }
      HIP_TRY(hipGetLastError());
    }
    /* the buffers just written become the input; the other scratch pair
     * becomes the output (a fused first pass's input drops out here) */
    uint64_t* kdone = kout; kout = knext; knext = kdone; kin = kdone;
    uint32_t* idone = iout; iout = inext; inext = idone; iin = iout_pass;
    in_mode = 0;
  }

  if (prefix_low >= 0) {
    void* kdst = (out_keys && !key.validity) ? out_keys : nullptr;
    int dec_mode = (key.dtype == GPUQ_FLOAT64 ? 2 : 1) | (desc ? 4 : 0);
    { hipEvent_t _pe = prof_begin(s);
    k_sort_tiefix<<<dim3((uint32_t)sort_nblocks(n_sort, TIEFIX_TILE)), TIEFIX_BLOCK, 0, s>>>(
        n_sort, kin, iin, out_perm + sorted_at, (uint64_t*)kdst, prefix_low * 8,
        dec_mode, &w.err[1]);
    prof_end("sort_tiefix", s, _pe); }
    HIP_TRY(hipGetLastError());
  }

  if (onesweep || prefix_low >= 0) {
    /* one bounded-spin timeout check; on timeout redo with hist+scan (the
     * input was only read; pass buffers are scratch). The tie-fix overflow
     * word rides the same copy. */
    unsigned long long herr2[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(herr2, w.err, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long herr = onesweep ? herr2[0] : 0;
    if (!herr && prefix_low >= 0 && herr2[1]) {
      /* a run longer than GPUQ_SORT_TIE_MAX was not in order: redo with
       * today's full pass list (same re-encode rules as the timeout path) */
      g_sort_plan.fell_back = 1;
      no_prefix = true;
      if (key.validity) {
        sort_plan_rec tried = g_sort_plan;
        force_no_prefix = 1;
        int rc = gpuq_sort_perm(stream, n, key, desc, nulls_first, out_perm,
                                out_keys, workspace, workspace_bytes);
        force_no_prefix = 0;
        g_sort_plan = tried;
        return rc;
      }
      /* fused: the raw column is intact and the redo's first pass reads it
       * again; otherwise ka/ia were consumed as scratch — re-encode */
      if (!fused) {
        launch_encode(s, n_sort, key.data, nullptr, key.dtype, desc, &w);
        HIP_TRY(hipGetLastError());
      }
      goto retry;
    }
    if (herr) {
      if (++retries > 1) FAIL(GPUQ_ERR_HIP, "sort: lookback timed out twice");
      onesweep = false;
      /* re-encode (ka/ia were consumed as ping-pong scratch; with a validity
       * split the rowmap in w.ib was also consumed -> rebuild is only needed
       * for the null-free path; with validity, fall back to a full redo) */
      if (key.validity) {
        force_classic = 1;
        int rc = gpuq_sort_perm(stream, n, key, desc, nulls_first, out_perm,
                                out_keys, workspace, workspace_bytes);
        force_classic = 0;
        return rc;
      }
      /* hist+scan is unfused: materialise the pairs (also when the timed-out
       * attempt was fused and never wrote ka/ia) */
      fused = false;
      launch_encode(s, n_sort, key.data, nullptr, key.dtype, desc, &w);
      HIP_TRY(hipGetLastError());
      goto retry;
    }
  }
  if (last_byte < 0)  /* zero passes: identity permutation */
    HIP_TRY(hipMemcpyAsync(out_perm + sorted_at, iin, n_sort * 4, hipMemcpyDeviceToDevice, s));
  if (out_keys) {
    if (key.validity) {
      /* null rows' data values are whatever the input held — gather the
       * whole column by the final permutation */
      gpuq_col kc = key; kc.validity = nullptr;
      int rc = gpuq_gather(stream, n, kc, out_perm, out_keys);
      if (rc) return rc;
    } else if (last_byte >= 0) {
      /* keys were decoded by the fused final pass */
    } else {
      if (key.dtype == GPUQ_FLOAT64) {
        if (desc) k_decode<GPUQ_FLOAT64, true><<<grid1d(n), 256, 0, s>>>(n, kin, out_keys);
        else      k_decode<GPUQ_FLOAT64, false><<<grid1d(n), 256, 0, s>>>(n, kin, out_keys);
      } else {
        if (desc) k_decode<GPUQ_INT64, true><<<grid1d(n), 256, 0, s>>>(n, kin, out_keys);
        else      k_decode<GPUQ_INT64, false><<<grid1d(n), 256, 0, s>>>(n, kin, out_keys);
      }
      HIP_TRY(hipGetLastError());
    }
  }
  return GPUQ_OK;
}

/* ================= top-k (radix select) ================= */
/*
 * TakeOrderedAndProjectExec (execution/limit.scala) keeps the first k rows of
 * a sort order. Instead of sorting everything, an MSB radix select finds the
 * k-th key of the sort's own encoding (sort_in_word), then one stable stream
 * compaction emits the rows before it plus the boundary ties.
 *
 *  level   k_topk_hist: 256-bin histogram of one key byte over the rows whose
 *          higher bytes equal the prefix fixed so far. The host copies the
 *          256 counts, picks the digit that holds the remaining rank and
 *          moves to the next active byte (bytes uniform over the column are
 *          skipped by the sort's bits_changed rule; the first level produces
 *          that reduction and the NULL count).
 *  collect k_topk_collect: once the surviving bucket has at most
 *          TOPK_COMPACT_MAX rows, the same streaming read also appends the
 *          bucket's encoded keys to a workspace buffer; later levels read
 *          that buffer instead of the column.
 *  emit    k_topk_count + exclusive_scan_u32 + k_topk_emit: per-block counts
 *          of (before, tie) rows, their prefix sums, then a ranked write of
 *          the selected row ids in input order.
 */

#define TOPK_COMPACT_MAX (1 << 20)
#define TOPK_BLOCK 256
#define TOPK_WAVES (TOPK_BLOCK / WAVE)
#define TOPK_EMIT_ITEMS 8
#define TOPK_EMIT_TILE (TOPK_BLOCK * TOPK_EMIT_ITEMS) /* 2048 rows per block */

/* row classes of the emit: before the tie group T, in T, after T */
#define TOPK_BEFORE 0
#define TOPK_TIE 1
#define TOPK_AFTER 2

/* one LDS histogram increment per calling lane. When every calling lane of
 * the wave hits the same bin (a byte that is almost uniform, such as the
 * exponent byte of unit-range doubles) one lane adds the lane count instead
 * of 64 serialised same-address atomics. */
DEV void topk_hist_add(uint32_t* h, int bin) {
  unsigned long long act = __ballot(1);
  int b0 = __builtin_amdgcn_readfirstlane(bin);
  unsigned long long same = __ballot(bin == b0);
  if (same == act) {
    if ((int)__lane_id() == __ffsll((long long)act) - 1)
      atomicAdd(&h[b0], (uint32_t)__popcll(act));
  } else {
    atomicAdd(&h[bin], 1u);
  }
}

/* One select level. src holds raw keys (key_mode per sort_in_word) with an
 * optional validity bitmap, or the collected encoded keys (key_mode 0, no
 * bitmap). Counts byte `shift/8` of every valid row with
 * ((e ^ prefix) & mask) == 0 into ghist[256] (one global atomic per block
 * and non-zero bin). stats != nullptr (first level): also the AND / OR
 * reduction over the valid rows and the NULL count, stats = {and, or, nnull}.
 * Four keys per thread are in flight per iteration, as in k_encode. */
__global__ __launch_bounds__(TOPK_BLOCK)
void k_topk_hist(int64_t n, const uint64_t* src, const uint8_t* validity,
                 int key_mode, uint64_t prefix, uint64_t mask, int shift,
                 uint32_t* ghist, unsigned long long* stats) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  uint64_t acc_or = 0, acc_and = ~0ULL;
  uint32_t nulls = 0;
  int64_t i = (int64_t)blockIdx.x * TOPK_BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TOPK_BLOCK;
  for (; i + 3 * stride < n; i += 4 * stride) {
    uint64_t raw[4];
    bool ok[4];
    #pragma unroll
    for (int u = 0; u < 4; u++) {
      raw[u] = src[i + u * stride];
      ok[u] = bit_valid(validity, i + u * stride);
    }
    #pragma unroll
    for (int u = 0; u < 4; u++) {
      if (!ok[u]) { nulls++; continue; }
      uint64_t e = sort_in_word(raw[u], key_mode);
      acc_or |= e; acc_and &= e;
      if (((e ^ prefix) & mask) == 0) topk_hist_add(h, (int)((e >> shift) & 0xff));
    }
  }
  for (; i < n; i += stride) {
    if (!bit_valid(validity, i)) { nulls++; continue; }
    uint64_t e = sort_in_word(src[i], key_mode);
    acc_or |= e; acc_and &= e;
    if (((e ^ prefix) & mask) == 0) topk_hist_add(h, (int)((e >> shift) & 0xff));
  }
  if (stats) {
    /* wave reduce then one atomic per wave (G12) */
    for (int off = 32; off > 0; off >>= 1) {
      acc_or |= __shfl_down((unsigned long long)acc_or, off);
      acc_and &= __shfl_down((unsigned long long)acc_and, off);
      nulls += __shfl_down(nulls, off);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      atomicAnd(&stats[0], (unsigned long long)acc_and);
      atomicOr(&stats[1], (unsigned long long)acc_or);
      if (nulls) atomicAdd(&stats[2], (unsigned long long)nulls);
    }
  }
  __syncthreads();
  uint32_t v = h[threadIdx.x];
  if (v) atomicAdd(&ghist[threadIdx.x], v);
}

/* Bucket compaction fused with the next level: every valid row of the column
 * with ((e ^ prefix) & mask) == 0 is appended (encoded) to cbuf — order is
 * irrelevant to a histogram — and counted into ghist by byte `shift/8`.
 * A block walks tiles of TOPK_COLLECT_TILE consecutive rows, stages its
 * matches in LDS (one LDS bump per wave) and flushes the stage with ONE bump
 * of the global cursor and coalesced stores whenever another tile might not
 * fit, so the cursor sees one returning atomic per ~1-2 K collected rows, not
 * one per wave. cap is the bucket size the previous level counted; the bound
 * on the write only matters if the caller broke the contract and changed the
 * column meanwhile. */
#define TOPK_COLLECT_ITEMS 4
#define TOPK_COLLECT_TILE (TOPK_BLOCK * TOPK_COLLECT_ITEMS) /* 1024 */
#define TOPK_STAGE (2 * TOPK_COLLECT_TILE)

__global__ __launch_bounds__(TOPK_BLOCK)
void k_topk_collect(int64_t n, const uint64_t* src, const uint8_t* validity,
                    int key_mode, uint64_t prefix, uint64_t mask, int shift,
                    uint32_t* ghist, uint64_t* cbuf, unsigned int* cursor,
                    uint32_t cap) {
  __shared__ uint32_t h[256];
  __shared__ uint64_t stage[TOPK_STAGE];
  __shared__ uint32_t staged, gbase;
  h[threadIdx.x] = 0;
  if (threadIdx.x == 0) staged = 0;
  __syncthreads();
  const unsigned long long lt = (1ULL << __lane_id()) - 1;
  /* called by the whole block, after a barrier that follows the last add */
  auto flush = [&]() {
    if (threadIdx.x == 0) gbase = staged ? atomicAdd(cursor, staged) : 0;
    __syncthreads();
    uint32_t cnt = staged, gb = gbase;
    for (uint32_t j = threadIdx.x; j < cnt; j += TOPK_BLOCK)
      if (gb + j < cap) cbuf[gb + j] = stage[j];
    __syncthreads();
    if (threadIdx.x == 0) staged = 0;
    __syncthreads();
  };
  /* the trip count depends on blockIdx only: every barrier below is uniform */
  for (int64_t base = (int64_t)blockIdx.x * TOPK_COLLECT_TILE; base < n;
       base += (int64_t)gridDim.x * TOPK_COLLECT_TILE) {
    uint64_t raw[TOPK_COLLECT_ITEMS];
    bool ok[TOPK_COLLECT_ITEMS];
    #pragma unroll
    for (int u = 0; u < TOPK_COLLECT_ITEMS; u++) {
      int64_t i = base + u * TOPK_BLOCK + threadIdx.x;
      ok[u] = i < n && bit_valid(validity, i);
      raw[u] = i < n ? src[i] : 0;
    }
    #pragma unroll
    for (int u = 0; u < TOPK_COLLECT_ITEMS; u++) {
      uint64_t e = sort_in_word(raw[u], key_mode);
      if (ok[u] && ((e ^ prefix) & mask) == 0) {
        unsigned long long act = __ballot(1);
        uint32_t rank = (uint32_t)__popcll(act & lt);
        uint32_t slot = 0;
        if (rank == 0) slot = atomicAdd(&staged, (uint32_t)__popcll(act));
        slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot) + rank;
        stage[slot] = e;   /* < TOPK_STAGE: at most one tile since the last check */
        topk_hist_add(h, (int)((e >> shift) & 0xff));
      }
    }
    __syncthreads();
    uint32_t have = staged;
    __syncthreads();   /* nobody adds again before everyone has read `have` */
    if (have > TOPK_STAGE - TOPK_COLLECT_TILE) flush();
  }
  flush();
  uint32_t v = h[threadIdx.x];
  if (v) atomicAdd(&ghist[threadIdx.x], v);
}

/* class of row i against the threshold: NULL rows take null_class; valid rows
 * take valid_class when it is >= 0 (T is the NULL group), else compare. */
DEV int topk_class(const uint64_t* keys, const uint8_t* validity, int64_t i,
                   int key_mode, uint64_t thr, int null_class, int valid_class) {
  uint64_t e = sort_in_word(keys[i], key_mode);
  if (!bit_valid(validity, i)) return null_class;
  if (valid_class >= 0) return valid_class;
  return e < thr ? TOPK_BEFORE : (e == thr ? TOPK_TIE : TOPK_AFTER);
}

/* emit phase 1: block b counts the before / tie rows of its tile of
 * TOPK_EMIT_TILE consecutive rows into cnt[b] / cnt[nblocks + b]. */
__global__ __launch_bounds__(TOPK_BLOCK)
void k_topk_count(int64_t n, const uint64_t* keys, const uint8_t* validity,
                  int key_mode, uint64_t thr, int null_class, int valid_class,
                  uint32_t* cnt, uint32_t nblocks) {
  __shared__ uint32_t c[2];
  if (threadIdx.x < 2) c[threadIdx.x] = 0;
  __syncthreads();
  int64_t base = (int64_t)blockIdx.x * TOPK_EMIT_TILE;
  uint32_t nb = 0, nt = 0;
  #pragma unroll
  for (int r = 0; r < TOPK_EMIT_ITEMS; r++) {
    int64_t i = base + r * TOPK_BLOCK + threadIdx.x;
    int cls = i < n ? topk_class(keys, validity, i, key_mode, thr, null_class, valid_class)
                    : TOPK_AFTER;
    nb += cls == TOPK_BEFORE;
    nt += cls == TOPK_TIE;
  }
  for (int off = 32; off > 0; off >>= 1) {
    nb += __shfl_down(nb, off);
    nt += __shfl_down(nt, off);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (nb) atomicAdd(&c[0], nb);
    if (nt) atomicAdd(&c[1], nt);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = c[0];
    cnt[nblocks + blockIdx.x] = c[1];
  }
}

/* emit phase 2: scan is the exclusive prefix sum of cnt, so scan[b] is the
 * number of before rows ahead of block b and scan[nblocks + b] - n_before_rows
 * the number of tie rows ahead of it. A before row is always written; a tie
 * row when its ordinal within T is below tie_take (|T| with keep_ties). With
 * bb / tt the before / tie rows ahead of a row inside its block, the row's
 * slot is before_prefix + bb + min(tie_prefix + tt, tie_take): ascending row
 * ids. In-block ranks: wave ballot + popcount, then an LDS scan over the
 * waves (double-buffered by round parity: one barrier per round). */
__global__ __launch_bounds__(TOPK_BLOCK)
void k_topk_emit(int64_t n, const uint64_t* keys, const uint8_t* validity,
                 int key_mode, uint64_t thr, int null_class, int valid_class,
                 const uint32_t* scan, uint32_t nblocks, uint32_t n_before_rows,
                 uint32_t tie_take, uint32_t* out_rids, int64_t out_capacity) {
  __shared__ uint32_t wtot[2][TOPK_WAVES][2];
  const int wave = threadIdx.x / WAVE;
  const unsigned long long lt = (1ULL << (threadIdx.x & (WAVE - 1))) - 1;
  int64_t base = (int64_t)blockIdx.x * TOPK_EMIT_TILE;
  int cls[TOPK_EMIT_ITEMS];
  #pragma unroll
  for (int r = 0; r < TOPK_EMIT_ITEMS; r++) {
    int64_t i = base + r * TOPK_BLOCK + threadIdx.x;
    cls[r] = i < n ? topk_class(keys, validity, i, key_mode, thr, null_class, valid_class)
                   : TOPK_AFTER;
  }
  uint32_t run_b = scan[blockIdx.x];
  uint32_t run_t = scan[nblocks + blockIdx.x] - n_before_rows;
  #pragma unroll
  for (int r = 0; r < TOPK_EMIT_ITEMS; r++) {
    unsigned long long mb = __ballot(cls[r] == TOPK_BEFORE);
    unsigned long long mt = __ballot(cls[r] == TOPK_TIE);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      wtot[r & 1][wave][0] = (uint32_t)__popcll(mb);
      wtot[r & 1][wave][1] = (uint32_t)__popcll(mt);
    }
    __syncthreads();
    uint32_t bb = run_b + (uint32_t)__popcll(mb & lt);
    uint32_t tt = run_t + (uint32_t)__popcll(mt & lt);
    #pragma unroll
    for (int w = 0; w < TOPK_WAVES; w++) {
      uint32_t wb = wtot[r & 1][w][0], wt = wtot[r & 1][w][1];
      if (w < wave) { bb += wb; tt += wt; }
      run_b += wb; run_t += wt;
    }
    bool sel = cls[r] == TOPK_BEFORE || (cls[r] == TOPK_TIE && tt < tie_take);
    if (sel) {
      int64_t pos = (int64_t)bb + (tt < tie_take ? tt : tie_take);
      if (pos < out_capacity)
        out_rids[pos] = (uint32_t)(base + r * TOPK_BLOCK + threadIdx.x);
    }
  }
}

struct topk_ws {
  uint64_t* cbuf;            /* collected encoded keys of the bucket */
  uint32_t* hist;            /* [256] level histogram */
  unsigned long long* stats; /* {and, or, nnull, collect cursor} */
  uint32_t* cnt;             /* [2][emit blocks] before / tie counts */
  uint32_t* scan;            /* exclusive prefix sums of cnt */
  uint32_t* block_sums;
};

static void topk_ws_layout(int64_t n, topk_ws* w, char* basep, int64_t* total) {
  int64_t nb = (n + TOPK_EMIT_TILE - 1) / TOPK_EMIT_TILE;
  int64_t scan_blocks = (2 * nb + SCAN_TILE - 1) / SCAN_TILE + 1;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = basep ? basep + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->cbuf = (uint64_t*)take((n < TOPK_COMPACT_MAX ? n : TOPK_COMPACT_MAX) * 8);
  w->hist = (uint32_t*)take(256 * 4);
  w->stats = (unsigned long long*)take(4 * 8);
  w->cnt = (uint32_t*)take(2 * nb * 4);
  w->scan = (uint32_t*)take(2 * nb * 4);
  w->block_sums = (uint32_t*)take(scan_blocks * 4);
  *total = off;
}

extern "C" int64_t gpuq_topk_workspace_bytes(int64_t n) {
  if (n < 0) n = 0;
  topk_ws w; int64_t total;
  topk_ws_layout(n, &w, nullptr, &total);
  return total;
}

extern "C" int gpuq_topk_candidates(void* stream, int64_t n, gpuq_col key,
                                    int32_t desc, int32_t nulls_first, int64_t k,
                                    int32_t keep_ties,
                                    uint32_t* out_rids, int64_t out_capacity,
                                    int64_t* out_counts,
                                    void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  out_counts[0] = out_counts[1] = out_counts[2] = 0;
  if (n < 0 || n > 0xFFFFFFFFLL)
    FAIL(GPUQ_ERR_INVALID, "topk: nrows %lld out of range", (long long)n);
  if (key.dtype != GPUQ_INT64 && key.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "topk: unsupported dtype %d", key.dtype);
  topk_ws w; int64_t need;
  topk_ws_layout(n, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "topk: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
  if (k <= 0 || n == 0) return GPUQ_OK;

  const int64_t kk = k < n ? k : n;   /* rows wanted */
  const int64_t pos = kk - 1;         /* position in S that defines T */
  const int key_mode = (key.dtype == GPUQ_FLOAT64 ? 2 : 1) | (desc ? 4 : 0);
  const uint64_t* col = (const uint64_t*)key.data;
  uint32_t hh[256];
  unsigned long long hs[3];

  /* level 0: top byte, plus the AND/OR reduction and the NULL count */
  HIP_TRY(hipMemsetAsync(w.hist, 0, 256 * 4, s));
  HIP_TRY(hipMemsetAsync(w.stats, 0, 32, s));
  HIP_TRY(hipMemsetAsync(w.stats, 0xFF, 8, s));  /* bits_and = ~0 */
  { hipEvent_t _pe = prof_begin(s);
  k_topk_hist<<<grid1d(n, TOPK_BLOCK), TOPK_BLOCK, 0, s>>>(
      n, col, key.validity, key_mode, 0, 0, 56, w.hist, w.stats);
  prof_end("topk_hist", s, _pe); }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hh, w.hist, sizeof(hh), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hs, w.stats, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t nnull = (int64_t)hs[2], nvalid = n - nnull;
  if (nnull < 0 || nnull > n) FAIL(GPUQ_ERR_INVALID, "topk: bad NULL count");

  /* NULLs are one group at the head or the tail of S */
  const bool t_is_null = nulls_first ? pos < nnull : pos >= nvalid;
  int64_t n_before, n_tie;
  uint64_t thr = 0;
  int null_class, valid_class;
  if (t_is_null) {
    n_before = nulls_first ? 0 : nvalid;
    n_tie = nnull;
    null_class = TOPK_TIE;
    valid_class = nulls_first ? TOPK_AFTER : TOPK_BEFORE;
  } else {
    const int64_t head = nulls_first ? nnull : 0;   /* NULLs ahead of the valid rows */
    int64_t r = pos - head;       /* remaining rank inside the current bucket */
    int64_t before = 0;           /* valid rows known to sort before the bucket */
    int64_t bucket = nvalid;
    const uint64_t bits_changed = hs[0] ^ hs[1];
    uint64_t prefix = hs[0];      /* uniform bytes are right already */
    const uint64_t* src = col;
    const uint8_t* src_valid = key.validity;
    int64_t n_src = n;
    int src_mode = key_mode;
    for (int b = 7; b >= 0; b--) {
      if (((bits_changed >> (b * 8)) & 0xff) == 0) continue;  /* uniform byte */
      if (b != 7) {   /* level 0 already counted byte 7 into hh */
        const uint64_t mask = ~0ULL << ((b + 1) * 8);
        HIP_TRY(hipMemsetAsync(w.hist, 0, 256 * 4, s));
        if (src == col && bucket <= TOPK_COMPACT_MAX) {
          { hipEvent_t _pe = prof_begin(s);
          k_topk_collect<<<grid1d(n, TOPK_BLOCK), TOPK_BLOCK, 0, s>>>(
              n, col, key.validity, key_mode, prefix, mask, b * 8, w.hist,
              w.cbuf, (unsigned int*)&w.stats[3], (uint32_t)bucket);
          prof_end("topk_collect", s, _pe); }
          src = w.cbuf; src_valid = nullptr; n_src = bucket; src_mode = 0;
        } else {
          { hipEvent_t _pe = prof_begin(s);
          k_topk_hist<<<grid1d(n_src, TOPK_BLOCK), TOPK_BLOCK, 0, s>>>(
              n_src, src, src_valid, src_mode, prefix, mask, b * 8, w.hist, nullptr);
          prof_end("topk_hist", s, _pe); }
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(hh, w.hist, sizeof(hh), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
      }
      int64_t cum = 0;
      int d = 0;
      for (; d < 256; d++) {
        if (r < cum + (int64_t)hh[d]) break;
        cum += hh[d];
      }
      if (d == 256)
        FAIL(GPUQ_ERR_INVALID, "topk: level counts do not add up (key column changed during the call?)");
      before += cum;
      r -= cum;
      bucket = hh[d];
      prefix = (prefix & ~(0xffULL << (b * 8))) | ((uint64_t)d << (b * 8));
    }
    thr = prefix;
    n_before = head + before;
    n_tie = bucket;
    null_class = nulls_first ? TOPK_BEFORE : TOPK_AFTER;
    valid_class = -1;
  }
  const int64_t tie_take = keep_ties ? n_tie : kk - n_before;
  if (tie_take < 1 || tie_take > n_tie)
    FAIL(GPUQ_ERR_INVALID, "topk: inconsistent counts (key column changed during the call?)");
  const int64_t n_cand = n_before + tie_take;
  out_counts[0] = n_cand; out_counts[1] = n_before; out_counts[2] = n_tie;
  if (n_cand > out_capacity)
    FAIL(GPUQ_ERR_OVERFLOW, "topk: %lld candidates > out_capacity %lld",
         (long long)n_cand, (long long)out_capacity);

  /* emit: per-block (before, tie) counts, one scan over both, ranked write */
  const int64_t nb = (n + TOPK_EMIT_TILE - 1) / TOPK_EMIT_TILE;
  hipEvent_t _pe = prof_begin(s);
  k_topk_count<<<dim3((uint32_t)nb), TOPK_BLOCK, 0, s>>>(
      n, col, key.validity, key_mode, thr, null_class, valid_class, w.cnt, (uint32_t)nb);
  HIP_TRY(hipGetLastError());
  int rc = exclusive_scan_u32(s, 2 * nb, w.cnt, w.scan, w.block_sums);
  if (rc) return rc;
  k_topk_emit<<<dim3((uint32_t)nb), TOPK_BLOCK, 0, s>>>(
      n, col, key.validity, key_mode, thr, null_class, valid_class, w.scan,
      (uint32_t)nb, (uint32_t)n_before, (uint32_t)tie_take, out_rids, out_capacity);
  prof_end("topk_emit", s, _pe);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ---- partition: one ranked-scatter pass with bin = partition id ---- */

/* pack (validity, key) into the u64 slot used by compute_bin<1>:
 * top bit set = NULL key; low 63 bits = key (keys needing bit 63 are rare
 * in partition keys? NO — must be exact: instead we pre-compute pids). */

/* For exactness with full-range int64 keys we precompute the pid array and
 * use BIN_MODE 0 over its low byte (num_parts <= 256). */
__global__ void k_partition_pids(int64_t n, const int64_t* keys, const uint8_t* validity,
                                 int32_t nparts, uint64_t* pid_as_key, uint32_t* idx,
                                 unsigned long long* counts /* [nparts] */) {
  __shared__ uint32_t h[256];
  bool lds_counts = nparts <= 256;
  if (lds_counts)
    for (int b = threadIdx.x; b < nparts; b += blockDim.x) h[b] = 0;
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int32_t hsh = 42;
    if (bit_valid(validity, i)) hsh = mm3_hash_long(keys[i], 42);
    int pid = spark_pmod(hsh, nparts);
    pid_as_key[i] = (uint64_t)pid;
    idx[i] = (uint32_t)i;
    if (lds_counts) atomicAdd(&h[pid], 1u);
    else atomicAdd(&counts[pid], 1ull);
  }
  __syncthreads();
  if (lds_counts)
    for (int b = threadIdx.x; b < nparts; b += blockDim.x)
      if (h[b]) atomicAdd(&counts[b], (unsigned long long)h[b]);
}

extern "C" int64_t gpuq_partition_workspace_bytes(int64_t n, int32_t nparts) {
  (void)nparts;
  sort_ws w; int64_t total;
  sort_ws_layout(n, 256, &w, nullptr, &total);
  return total;
}

extern "C" int gpuq_partition_perm(void* stream, int64_t n, gpuq_col key,
                                   int32_t nparts, uint32_t* out_perm,
                                   int64_t* out_counts,
                                   void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n > 0xFFFFFFFFLL) FAIL(GPUQ_ERR_INVALID, "partition: nrows %lld > 2^32", (long long)n);
  if (nparts < 1 || nparts > 65536)
    FAIL(GPUQ_ERR_INVALID, "partition: num_parts %d not in [1,65536]", nparts);
  if (key.dtype != GPUQ_INT64) FAIL(GPUQ_ERR_INVALID, "partition: key must be int64");
  sort_ws w; int64_t need;
  sort_ws_layout(n, 256, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "partition: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
  HIP_TRY(hipMemsetAsync(out_counts, 0, (size_t)nparts * 8, s));
  if (n == 0) return GPUQ_OK;
  { hipEvent_t _pe = prof_begin(s);
    k_partition_pids<<<grid1d(n), 256, 0, s>>>(n, (const int64_t*)key.data, key.validity,
                                             nparts, w.ka, w.ia,
                                             (unsigned long long*)out_counts);
    prof_end("partition_pids", s, _pe); }
  HIP_TRY(hipGetLastError());
  scatter_geom geom = get_sort_geom();
  int tile = geom.block * geom.items;
  int64_t nb = sort_nblocks(n, tile);
  /* stable LSB radix over the pid: one 8-bit pass, two when nparts > 256 */
  int passes = nparts > 256 ? 2 : 1;
  uint64_t *kin = w.ka, *kout = w.kb;
  uint32_t *iin = w.ia, *iout = w.ib;
  for (int p = 0; p < passes; p++) {
    { hipEvent_t _pe = prof_begin(s);
    k_radix_hist<0><<<dim3((uint32_t)nb), 256, 0, s>>>(n, kin, p * 8, w.hist, (int)nb, tile);
    prof_end("radix_hist", s, _pe); }
    HIP_TRY(hipGetLastError());
    int rc = exclusive_scan_u32(s, (int64_t)256 * nb, w.hist, w.hist_scan, w.block_sums);
    if (rc) return rc;
    uint32_t* iout_pass = (p == passes - 1) ? out_perm : iout;
    { hipEvent_t _pe = prof_begin(s);
    launch_scatter<0, false>(s, geom, nb, n, kin, iin, kout, iout_pass, w.hist_scan,
                             p * 8, 0, nullptr, nullptr, nullptr, 0);
    prof_end("radix_scatter", s, _pe); }
    HIP_TRY(hipGetLastError());
    uint64_t* tk = kin; kin = kout; kout = tk;
    uint32_t* ti = iin; iin = iout_pass; iout = ti;
  }
  return GPUQ_OK;
}

/* ---- range partition: bin = first bound >= key (RangePartitioning,
 * exchange/ShuffleExchangeExec.scala:379-400: sampled bounds, keys <= 
 * bounds[j] stay in partition j; partition order follows the sort order,
 * so a per-rank sort after the exchange yields a globally ordered
 * rank-major result). Keys and bounds are radix-encoded with the SAME
 * encoding as the sort (desc = complement), so ascending logic covers
 * both directions. NULL keys go to the first (nulls_first) or last
 * partition, matching SortOrder null placement. nbounds <= 2047. */
__global__ void k_range_pids(int64_t n, const void* keys, const uint8_t* validity,
                             int dtype, int desc, int nulls_first,
                             const void* bounds, int nbounds,
                             uint64_t* pid_as_key, uint32_t* idx,
                             unsigned long long* counts /* [nbounds+1] */) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long eb[];
  for (int j = threadIdx.x; j < nbounds; j += blockDim.x) {
    uint64_t e = (dtype == GPUQ_FLOAT64) ? encode_f64(((const double*)bounds)[j])
                                         : encode_i64(((const int64_t*)bounds)[j]);
    eb[j] = desc ? ~e : e;
  }
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int pid;
    if (!bit_valid(validity, i)) {
      pid = nulls_first ? 0 : nbounds;
    } else {
      uint64_t e = (dtype == GPUQ_FLOAT64) ? encode_f64(((const double*)keys)[i])
                                           : encode_i64(((const int64_t*)keys)[i]);
      if (desc) e = ~e;
      int lo = 0, hi = nbounds;          /* first j with e <= eb[j] */
      while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (e <= eb[mid]) hi = mid; else lo = mid + 1;
      }
      pid = lo;
    }
    pid_as_key[i] = (uint64_t)pid;
    idx[i] = (uint32_t)i;
    atomicAdd(&counts[pid], 1ull);
  }
}

extern "C" int gpuq_range_partition_perm(void* stream, int64_t n, gpuq_col key,
                                         int32_t desc, int32_t nulls_first,
                                         const void* bounds, int32_t nbounds,
                                         uint32_t* out_perm, int64_t* out_counts,
                                         void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n > 0xFFFFFFFFLL) FAIL(GPUQ_ERR_INVALID, "range_partition: nrows %lld > 2^32", (long long)n);
  if (nbounds < 0 || nbounds > 2047)
    FAIL(GPUQ_ERR_INVALID, "range_partition: nbounds %d not in [0,2047]", nbounds);
  if (key.dtype != GPUQ_INT64 && key.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "range_partition: unsupported dtype %d", key.dtype);
  sort_ws w; int64_t need;
  sort_ws_layout(n, 256, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "range_partition: workspace %lld < %lld",
         (long long)workspace_bytes, (long long)need);
  HIP_TRY(hipMemsetAsync(out_counts, 0, (size_t)(nbounds + 1) * 8, s));
  if (n == 0) return GPUQ_OK;
  k_range_pids<<<grid1d(n), 256, (uint32_t)(nbounds * 8), s>>>(
      n, key.data, key.validity, key.dtype, desc, nulls_first, bounds, nbounds,
      w.ka, w.ia, (unsigned long long*)out_counts);
  HIP_TRY(hipGetLastError());
  scatter_geom geom = get_sort_geom();
  int tile = geom.block * geom.items;
  int64_t nb = sort_nblocks(n, tile);
  int passes = (nbounds + 1) > 256 ? 2 : 1;
  uint64_t *kin = w.ka, *kout = w.kb;
  uint32_t *iin = w.ia, *iout = w.ib;
  for (int p = 0; p < passes; p++) {
    k_radix_hist<0><<<dim3((uint32_t)nb), 256, 0, s>>>(n, kin, p * 8, w.hist, (int)nb, tile);
    HIP_TRY(hipGetLastError());
    int rc = exclusive_scan_u32(s, (int64_t)256 * nb, w.hist, w.hist_scan, w.block_sums);
    if (rc) return rc;
    uint32_t* iout_pass = (p == passes - 1) ? out_perm : iout;
    launch_scatter<0, false>(s, geom, nb, n, kin, iin, kout, iout_pass, w.hist_scan,
                             p * 8, 0, nullptr, nullptr, nullptr, 0);
    HIP_TRY(hipGetLastError());
    uint64_t* tk = kin; kin = kout; kout = tk;
    uint32_t* ti = iin; iin = iout_pass; iout = ti;
  }
  return GPUQ_OK;
}

/* ================= hash aggregate ================= */
/*
 * Open-address table, EMPTY key sentinel = -1 (memset 0xFF); rows whose key
 * IS -1 and NULL-key rows use dedicated special slots so the full int64
 * domain is exact. Linear probing on Murmur3(key,42) (the reference probes
 * the same hash with triangular steps, BytesToBytesMap.java:513-539 —
 * probe order is unobservable in results).
 * Workspace: [cap u64 keys][cap f64 sums][cap u64 counts][special block]
 */

#define AGG_EMPTY 0xFFFFFFFFFFFFFFFFULL

struct agg_special {
  double m1_sum;   unsigned long long m1_cnt;  unsigned long long m1_seen;
  double nul_sum;  unsigned long long nul_cnt; unsigned long long nul_seen;
  unsigned long long out_cursor;
  unsigned long long overflow;
};

/* Interleaved slots [key, sum-bits, count(, pad)] so one probe touches one
 * cache line instead of three parallel arrays. Stride (u64 words/slot) is
 * 3 (24 B, default) or 4 (32 B, never line-straddling) via GPUQ_AGG_STRIDE. */
static int agg_stride(void) {
  static int s = 0;
  if (!s) {
    const char* e = getenv("GPUQ_AGG_STRIDE");
    s = (e && atoi(e) == 4) ? 4 : 3;
  }
  return s;
}

struct agg_ws {
  unsigned long long* tab;   /* stride * cap u64 */
  agg_special* sp;
};

static void agg_ws_layout(int64_t cap, agg_ws* w, char* base, int64_t* total) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->tab = (unsigned long long*)take(cap * 8 * 4);  /* sized for stride 4 */
  w->sp = (agg_special*)take(sizeof(agg_special));
  *total = off;
}

extern "C" int64_t gpuq_hash_agg_workspace_bytes(int64_t cap) {
  agg_ws w; int64_t total;
  agg_ws_layout(cap, &w, nullptr, &total);
  return total;
}

template <int SLOT>
__global__ void k_agg_init(int64_t cap, unsigned long long* tab) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < cap; i += stride) {
    tab[SLOT * i] = AGG_EMPTY;
    tab[SLOT * i + 1] = 0;
    tab[SLOT * i + 2] = 0;
  }
}

#define AGG_OP_SUM 1
#define AGG_OP_COUNT 2

template <int OPS, int SLOT>
__global__ void k_agg_build(int64_t n, const int64_t* keys, const uint8_t* kvalid,
                            const double* vals, const uint8_t* vvalid,
                            unsigned long long* tab, agg_special* sp,
                            int64_t cap_mask) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    bool kv = bit_valid(kvalid, i);
    bool vv = bit_valid(vvalid, i);
    double v = vv ? vals[i] : 0.0;
    if (!kv || (unsigned long long)keys[i] == AGG_EMPTY) {
      double* psum = kv ? &sp->m1_sum : &sp->nul_sum;
      unsigned long long* pcnt = kv ? &sp->m1_cnt : &sp->nul_cnt;
      unsigned long long* pseen = kv ? &sp->m1_seen : &sp->nul_seen;
      atomicMax(pseen, 1ull);
      if (vv) {
        if (OPS & AGG_OP_SUM) atomicAdd(psum, v);
        if (OPS & AGG_OP_COUNT) atomicAdd(pcnt, 1ull);
      }
      continue;
    }
    int64_t k = keys[i];
    uint64_t slot = ((uint32_t)mm3_hash_long(k, 42)) & (uint64_t)cap_mask;
    for (int probes = 0;; probes++) {
      unsigned long long cur = __hip_atomic_load(&tab[SLOT * slot], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
      if (cur == (unsigned long long)k) break;
      if (cur == AGG_EMPTY) {
        unsigned long long prev = atomicCAS(&tab[SLOT * slot], AGG_EMPTY, (unsigned long long)k);
        if (prev == AGG_EMPTY || prev == (unsigned long long)k) break;
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
      if (probes > cap_mask) { atomicMax(&sp->overflow, 1ull); return; }
    }
    if (vv) {
      if (OPS & AGG_OP_SUM) atomicAdd((double*)&tab[SLOT * slot + 1], v);
      if (OPS & AGG_OP_COUNT) atomicAdd(&tab[SLOT * slot + 2], 1ull);
    }
  }
}

#define AGGC_CHUNK 8192

template <int OPS, int SLOT>
__global__ void k_agg_compact(int64_t cap, const unsigned long long* tab,
                              agg_special* sp,
                              int64_t* out_keys, uint8_t* out_kvalid,
                              double* out_sums, uint8_t* out_svalid,
                              int64_t* out_cnts) {
  /* ONE output-cursor atomic per block (a single cursor word saturates
   * near ~88 updates/us): count occupied slots in this block's chunk,
   * block-scan, reserve once, emit. */
  constexpr int ROUNDS = AGGC_CHUNK / 256;
  __shared__ unsigned long long block_base;
  __shared__ uint32_t wtot[4];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t base = (int64_t)blockIdx.x * AGGC_CHUNK;
  uint32_t occ_mask[ROUNDS / 32 + 1];
  for (int m = 0; m < ROUNDS / 32 + 1; m++) occ_mask[m] = 0;
  uint32_t lane_total = 0;
  for (int r = 0; r < ROUNDS; r++) {
    int64_t i = base + r * 256 + threadIdx.x;
    bool occ = i < cap && tab[SLOT * i] != AGG_EMPTY;
    if (occ) { occ_mask[r / 32] |= 1u << (r & 31); lane_total++; }
  }
  uint32_t incl = wave_inclusive_scan(lane_total);
  if (lane == WAVE - 1) wtot[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int w = 0; w < 4; w++) { uint32_t t = wtot[w]; wtot[w] = tot; tot += t; }
    block_base = tot ? atomicAdd(&sp->out_cursor, (unsigned long long)tot) : 0;
  }
  __syncthreads();
  int64_t o = (int64_t)block_base + wtot[wave] + (incl - lane_total);
  for (int r = 0; r < ROUNDS; r++) {
    if (!((occ_mask[r / 32] >> (r & 31)) & 1)) continue;
    int64_t i = base + r * 256 + threadIdx.x;
    unsigned long long k = tab[SLOT * i];
    out_keys[o] = (int64_t)k;
    out_kvalid[o] = 1;
    out_sums[o] = __longlong_as_double((long long)tab[SLOT * i + 1]);
    out_svalid[o] = (OPS & AGG_OP_COUNT) ? (tab[SLOT * i + 2] > 0 ? 1 : 0) : 1;
    if (out_cnts) out_cnts[o] = (int64_t)tab[SLOT * i + 2];
    o++;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (sp->m1_seen) {
      int64_t q = (int64_t)atomicAdd(&sp->out_cursor, 1ull);
      out_keys[q] = -1; out_kvalid[q] = 1;
      out_sums[q] = sp->m1_sum;
      out_svalid[q] = (OPS & AGG_OP_COUNT) ? (sp->m1_cnt > 0 ? 1 : 0) : 1;
      if (out_cnts) out_cnts[q] = (int64_t)sp->m1_cnt;
    }
    if (sp->nul_seen) {
      int64_t q = (int64_t)atomicAdd(&sp->out_cursor, 1ull);
      out_keys[q] = 0; out_kvalid[q] = 0;
      out_sums[q] = sp->nul_sum;
      out_svalid[q] = (OPS & AGG_OP_COUNT) ? (sp->nul_cnt > 0 ? 1 : 0) : 1;
      if (out_cnts) out_cnts[q] = (int64_t)sp->nul_cnt;
    }
  }
}

/* small-cardinality build: per-block LDS table (classic two-level
 * aggregation), merged once into the global table per block. Removes the
 * global-atomic contention wall on few-group aggregates (measured 607 ms
 * for 1B rows / 1K groups on the direct path). cap <= AGG_LDS_CAP slots. */
#define AGG_LDS_CAP 2048

template <int OPS, int SLOT>
__global__ __launch_bounds__(256)
void k_agg_build_lds(int64_t n, const int64_t* keys, const uint8_t* kvalid,
                     const double* vals, const uint8_t* vvalid,
                     unsigned long long* tab, agg_special* sp,
                     int64_t cap_mask) {
  __shared__ unsigned long long lt[AGG_LDS_CAP * 3];
  const int64_t lcap = cap_mask + 1;
  for (int j = threadIdx.x; j < (int)lcap; j += blockDim.x) {
    lt[3 * j] = AGG_EMPTY; lt[3 * j + 1] = 0; lt[3 * j + 2] = 0;
  }
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    bool kv = bit_valid(kvalid, i);
    bool vv = bit_valid(vvalid, i);
    double v = vv ? vals[i] : 0.0;
    if (!kv || (unsigned long long)keys[i] == AGG_EMPTY) {
      double* psum = kv ? &sp->m1_sum : &sp->nul_sum;
      unsigned long long* pcnt = kv ? &sp->m1_cnt : &sp->nul_cnt;
      unsigned long long* pseen = kv ? &sp->m1_seen : &sp->nul_seen;
      atomicMax(pseen, 1ull);
      if (vv) {
        if (OPS & AGG_OP_SUM) atomicAdd(psum, v);
        if (OPS & AGG_OP_COUNT) atomicAdd(pcnt, 1ull);
      }
      continue;
    }
    int64_t k = keys[i];
    uint64_t slot = ((uint32_t)mm3_hash_long(k, 42)) & (uint64_t)cap_mask;
    for (int probes = 0;; probes++) {
      unsigned long long cur = lt[3 * slot];
      if (cur == (unsigned long long)k) break;
      if (cur == AGG_EMPTY) {
        unsigned long long prev = atomicCAS(&lt[3 * slot], AGG_EMPTY,
                                            (unsigned long long)k);
        if (prev == AGG_EMPTY || prev == (unsigned long long)k) break;
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
      if (probes > cap_mask) { atomicMax(&sp->overflow, 1ull); return; }
    }
    if (vv) {
      if (OPS & AGG_OP_SUM) atomicAdd((double*)&lt[3 * slot + 1], v);
      if (OPS & AGG_OP_COUNT) atomicAdd(&lt[3 * slot + 2], 1ull);
    }
  }
  __syncthreads();
  /* merge this block's LDS table into the global one (same probe scheme) */
  for (int j = threadIdx.x; j < (int)lcap; j += blockDim.x) {
    unsigned long long k = lt[3 * j];
    if (k == AGG_EMPTY) continue;
    uint64_t slot = ((uint32_t)mm3_hash_long((int64_t)k, 42)) & (uint64_t)cap_mask;
    /* the global table can be full of other blocks' keys even when no
     * block's own table overflowed: bound the probe and report, as the
     * direct build does, instead of probing forever */
    bool placed = true;
    for (int64_t probes = 0;; probes++) {
      unsigned long long cur = __hip_atomic_load(&tab[SLOT * slot], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
      if (cur == k) break;
      if (cur == AGG_EMPTY) {
        unsigned long long prev = atomicCAS(&tab[SLOT * slot], AGG_EMPTY, k);
        if (prev == AGG_EMPTY || prev == k) break;
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
      if (probes > cap_mask) { atomicMax(&sp->overflow, 1ull); placed = false; break; }
    }
    if (!placed) continue;
    if (OPS & AGG_OP_SUM)
      atomicAdd((double*)&tab[SLOT * slot + 1],
                __longlong_as_double((long long)lt[3 * j + 1]));
    if (OPS & AGG_OP_COUNT) atomicAdd(&tab[SLOT * slot + 2], lt[3 * j + 2]);
  }
}

extern "C" int gpuq_hash_agg_i64_f64(void* stream, int64_t n,
                                     gpuq_col key, gpuq_col val,
                                     void* workspace, int64_t cap, int32_t first_batch,
                                     int32_t finalize, int32_t ops,
                                     int64_t* out_keys, uint8_t* out_key_valid,
                                     double* out_sums, uint8_t* out_sum_valid,
                                     int64_t* out_counts, int64_t* out_ngroups) {
  hipStream_t s = (hipStream_t)stream;
  if (cap <= 0 || (cap & (cap - 1)))
    FAIL(GPUQ_ERR_INVALID, "agg: capacity %lld not a power of two", (long long)cap);
  if (key.dtype != GPUQ_INT64 || val.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "agg: expected int64 key + float64 val");
  if (!(ops & AGG_OP_COUNT) && val.validity)
    FAIL(GPUQ_ERR_INVALID, "agg: SUM-only mode requires non-null values "
         "(sum NULL-ness needs COUNT)");
  agg_ws w; int64_t need;
  agg_ws_layout(cap, &w, (char*)workspace, &need);
  if (first_batch) {
    if (agg_stride() == 4) k_agg_init<4><<<grid1d(cap), 256, 0, s>>>(cap, w.tab);
    else k_agg_init<3><<<grid1d(cap), 256, 0, s>>>(cap, w.tab);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(w.sp, 0, sizeof(agg_special), s));
  }
  if (n > 0) {
    { hipEvent_t _pe = prof_begin(s);
    bool lds_path = cap <= AGG_LDS_CAP && getenv("GPUQ_NO_LDS_AGG") == nullptr;
#define AGB(OPS, SL) k_agg_build<OPS, SL><<<hash_grid(n), 256, 0, s>>>( \
        n, (const int64_t*)key.data, key.validity, \
        (const double*)val.data, val.validity, w.tab, w.sp, cap - 1)
#define AGBL(OPS, SL) k_agg_build_lds<OPS, SL><<<hash_grid(n), 256, 0, s>>>( \
        n, (const int64_t*)key.data, key.validity, \
        (const double*)val.data, val.validity, w.tab, w.sp, cap - 1)
    if (lds_path) {
      if (agg_stride() == 4) { if (ops == AGG_OP_SUM) AGBL(AGG_OP_SUM, 4); else AGBL(3, 4); }
      else { if (ops == AGG_OP_SUM) AGBL(AGG_OP_SUM, 3); else AGBL(3, 3); }
    } else {
      if (agg_stride() == 4) { if (ops == AGG_OP_SUM) AGB(AGG_OP_SUM, 4); else AGB(3, 4); }
      else { if (ops == AGG_OP_SUM) AGB(AGG_OP_SUM, 3); else AGB(3, 3); }
    }
#undef AGB
#undef AGBL
    prof_end("agg_build", s, _pe); }
    HIP_TRY(hipGetLastError());
  }
  if (finalize) {
    agg_special hsp;
    HIP_TRY(hipMemcpyAsync(&hsp, w.sp, sizeof(hsp), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hsp.overflow) FAIL(GPUQ_ERR_OVERFLOW, "agg: hash table overflow (capacity %lld)", (long long)cap);
    { hipEvent_t _pe = prof_begin(s);
    dim3 cgrid((uint32_t)((cap + AGGC_CHUNK - 1) / AGGC_CHUNK));
#define AGC(OPS, SL) k_agg_compact<OPS, SL><<<cgrid, 256, 0, s>>>( \
        cap, w.tab, w.sp, out_keys, out_key_valid, out_sums, out_sum_valid, \
        out_counts)
    if (agg_stride() == 4) { if (ops == AGG_OP_SUM) AGC(AGG_OP_SUM, 4); else AGC(3, 4); }
    else { if (ops == AGG_OP_SUM) AGC(AGG_OP_SUM, 3); else AGC(3, 3); }
#undef AGC
    prof_end("agg_compact", s, _pe); }
    HIP_TRY(hipGetLastError());
    agg_special hsp2;
    HIP_TRY(hipMemcpyAsync(&hsp2, w.sp, sizeof(hsp2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out_ngroups = (int64_t)hsp2.out_cursor;
  }
  return GPUQ_OK;
}

/* ================= hash join ================= */
/*
 * Build: table of 16-byte interleaved slots {key u64, head u32, pad};
 * duplicates chained through next[] (the GPU analog of LongToUnsafeRowMap's
 * per-row next pointer, HashedRelation.scala:536-600), chain heads carry a
 * MULTI bit so single-match probes never read next[]. EMPTY key sentinel -1
 * with a dedicated chain for real -1 keys. NULL keys never match.
 *
 * Locality design (MI355X: random HBM lines are ~7x slower than L3-resident
 * access — measured in tools/diag_hash.py): the slot index is the TOP bits
 * of Murmur3(key,42) (multiplicative map, monotone in hash). The table is
 * flat and both sides are streamed in row order: radix-partitioning them
 * into hash order first was measured as net overhead once the output
 * cursor stopped being the bottleneck (the probe is latency-bound, not
 * line-refetch-bound) and was removed. Probe reserves output space with
 * one atomic per block.
 */

#define JOIN_NIL 0xFFFFFFFFu
#ifndef JOIN_CHUNK
#define JOIN_CHUNK 4096
#endif
#define JOIN_BLOCK 256   /* threads per build / probe block */

/* cursor sits at offset 8 (its natural alignment): joink_sp embeds this */
struct join_sp { unsigned int m1_head; unsigned long long cursor; };

/* hash -> slot: monotone multiplicative map onto [0, cap) */
DEV uint64_t join_slot(int64_t key, int64_t cap_mask) {
  uint32_t h = (uint32_t)mm3_hash_long(key, 42);
  return ((uint64_t)h * (uint64_t)(cap_mask + 1)) >> 32;
}

struct join_ws {
  unsigned long long* slots;   /* 2 u64 per slot: [key][head|pad] */
  unsigned int* next;
  unsigned long long* matched; /* build-row matched bits (full outer) */
  join_sp* sp;
};

static void join_ws_layout(int64_t cap, int64_t brows, join_ws* w, char* base, int64_t* total) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->slots = (unsigned long long*)take(cap * 16);
  w->next = (unsigned int*)take(brows * 4);
  w->matched = (unsigned long long*)take(((brows + 63) / 64) * 8);
  w->sp = (join_sp*)take(sizeof(join_sp));
  *total = off;
}

extern "C" int64_t gpuq_join_build_workspace_bytes(int64_t brows, int64_t cap) {
  join_ws w; int64_t total;
  join_ws_layout(cap, brows, &w, nullptr, &total);
  return total;
}

/* the probe needs no workspace of its own (kept for the ABI) */
extern "C" int64_t gpuq_join_probe_workspace_bytes(int64_t prows) {
  (void)prows;
  return 0;
}

/* chain-head word: bit 31 = MULTI (slot holds >1 row) so single-match
 * probes never touch next[]; low 31 bits = first build row index */
#define JOIN_MULTI 0x80000000u

DEV void join_push_head(unsigned int* headp, unsigned int i, unsigned int* next) {
  unsigned int old = __hip_atomic_load(headp, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    unsigned int newv = i | (old != JOIN_NIL ? JOIN_MULTI : 0u);
    unsigned int prev = atomicCAS(headp, old, newv);
    if (prev == old) {
      next[i] = (old == JOIN_NIL) ? JOIN_NIL : (old & ~JOIN_MULTI);
      break;
    }
    old = prev;
  }
}

/* contiguous-chunk mapping: block b owns rows [b*CHUNK, (b+1)*CHUNK) */
__global__ void k_join_build(int64_t n, const int64_t* keys, const uint8_t* kvalid,
                             unsigned long long* slots, unsigned int* next,
                             join_sp* sp, int64_t cap_mask) {
  int64_t base = (int64_t)blockIdx.x * JOIN_CHUNK;
  for (int r = 0; r < JOIN_CHUNK / 256; r++) {
    int64_t i = base + r * 256 + threadIdx.x;
    if (i >= n) return;
    if (!bit_valid(kvalid, i)) continue;  /* NULL never matches (inner join) */
    int64_t k = keys[i];
    if ((unsigned long long)k == AGG_EMPTY) {
      join_push_head(&sp->m1_head, (unsigned int)i, next);
      continue;
    }
    uint64_t slot = join_slot(k, cap_mask);
    for (;;) {
      unsigned long long cur = __hip_atomic_load(&slots[2 * slot], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
      if (cur == (unsigned long long)k) break;
      if (cur == AGG_EMPTY) {
        unsigned long long prev = atomicCAS(&slots[2 * slot], AGG_EMPTY, (unsigned long long)k);
        if (prev == AGG_EMPTY || prev == (unsigned long long)k) break;
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
    }
    join_push_head((unsigned int*)&slots[2 * slot + 1], (unsigned int)i, next);
  }
}

/* join types over the PROBE (streamed) side — the reference's
 * ShuffledHashJoinExec joinType dispatch (ShuffledHashJoinExec.scala /
 * HashJoin.scala join() : inner, outer, semi, anti):
 * 0 = Inner, 1 = probe-side Outer (unmatched probe rows emit one pair
 * with build rid = JOIN_NIL -> NULL build columns), 2 = LeftSemi (probe
 * row emitted once iff matched), 3 = LeftAnti (emitted iff unmatched;
 * NULL probe keys never match, so they emit — the non-null-aware anti). */
DEV uint32_t jt_emit_count(int jt, uint32_t m) {
  if (jt == 1 || jt == 4) return m ? m : 1u;  /* 4 = FullOuter probe half */
  if (jt == 2) return m ? 1u : 0u;
  if (jt == 3 || jt == 5) return m ? 0u : 1u; /* 5 = null-aware anti */
  return m;
}

/* ---- probe skeleton: k_join_probe, k_joink_probe and k_joink_probe_cond
 * differ only in how a row finds its chain head (join_find_head /
 * joink_find_head) and in which chain entries count as matches (the accept
 * functor: all of them, or joinc_pass) ----
 *
 * A block of JOIN_BLOCK threads owns CHUNK consecutive probe rows and takes
 * them in CHUNK / JOIN_BLOCK rounds. Phase A looks every row up, counts its
 * matches and keeps the first two (join_collect); ONE output-cursor atomic
 * per block then reserves the block's output (join_reserve: a single global
 * cursor word saturates near ~88 updates/us — the per-wave-iteration
 * version was the whole kernel's bottleneck); phase B emits (join_emit_row).
 * The kernels hold nothing but the two round loops. */

struct join_accept_all {
  __device__ bool operator()(int64_t, unsigned int) const { return true; }
};

/* Chain collect for probe row i: cnt = accepted entries of the chain at
 * `head`, c0 / c1 = the first two. Semi / anti need only "is there one", so
 * their walk stops at the first. */
template <int JT, class Accept>
DEV void join_collect(unsigned int head, int64_t i, const unsigned int* next,
                      unsigned long long* matched, Accept accept,
                      uint32_t* cnt, unsigned int* c0, unsigned int* c1) {
  uint32_t m = 0;
  unsigned int m0 = JOIN_NIL, m1 = JOIN_NIL;
  /* a head without JOIN_MULTI is a one-candidate chain: next[] untouched */
  const bool multi = head != JOIN_NIL && (head & JOIN_MULTI);
  for (unsigned int b = head == JOIN_NIL ? JOIN_NIL : (head & ~JOIN_MULTI);
       b != JOIN_NIL; b = multi ? next[b] : JOIN_NIL) {
    if (!accept(i, b)) continue;
    if (m == 0) m0 = b; else if (m == 1) m1 = b;
    m++;
    if (JT == 4) atomicOr(&matched[b >> 6], 1ull << (b & 63));
    if (JT == 2 || JT == 3 || JT == 5) break;
  }
  *cnt = m; *c0 = m0; *c1 = m1;
}

/* Block-level reservation of lane_total output slots per lane: returns this
 * lane's first slot (emit order within the block is arbitrary — join output
 * order is nondeterministic by contract). */
DEV int64_t join_reserve(uint32_t lane_total, unsigned long long* cursor) {
  __shared__ unsigned long long block_base;
  __shared__ uint32_t wtot[JOIN_BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  uint32_t incl = wave_inclusive_scan(lane_total);
  if (lane == WAVE - 1) wtot[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int w = 0; w < JOIN_BLOCK / WAVE; w++) {
      uint32_t t = wtot[w]; wtot[w] = tot; tot += t;
    }
    block_base = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0;
  }
  __syncthreads();
  return (int64_t)block_base + wtot[wave] + (incl - lane_total);
}

/* Emit probe row i's pairs from slot o on and advance o by what phase A
 * reserved for it. A row with more than two matches walks the rest of its
 * chain again, from next[c1] on, re-asking `accept`: both walks follow
 * next[] over an immutable table, so this one finds exactly the cnt - 2
 * entries phase A counted after c1. */
template <int JT, class Accept>
DEV void join_emit_row(int64_t i, bool in_range, uint32_t cnt, unsigned int c0,
                       unsigned int c1, const unsigned int* next, Accept accept,
                       int64_t& o, uint32_t* out_p, uint32_t* out_b,
                       int64_t out_cap) {
  if (JT != 0) {
    if (!in_range || !jt_emit_count(JT, cnt)) return;
    if (JT == 2 || JT == 3 || JT == 5 || cnt == 0) {
      /* semi/anti emit the probe row once; outer's unmatched row pairs
       * with NIL (NULL build columns downstream) */
      if (o < out_cap) { out_p[o] = (uint32_t)i; out_b[o] = JOIN_NIL; }
      o++;
      return;
    }
  }
  if (!cnt) return;
  if (o < out_cap) { out_p[o] = (uint32_t)i; out_b[o] = c0; }
  o++;
  if (cnt >= 2) {
    if (o < out_cap) { out_p[o] = (uint32_t)i; out_b[o] = c1; }
    o++;
  }
  if (cnt > 2) {
    /* o advances by the reserved cnt - 2 whatever the walk finds */
    const int64_t o_end = o + (cnt - 2);
    for (unsigned int b = next[c1]; b != JOIN_NIL && o < o_end; b = next[b]) {
      if (!accept(i, b)) continue;
      if (o < out_cap) { out_p[o] = (uint32_t)i; out_b[o] = b; }
      o++;
    }
    o = o_end;
  }
}

/* single-key lookup of a non-NULL key: open-address walk from join_slot, the
 * m1_head chain for real -1 keys (the slots' EMPTY sentinel) */
DEV unsigned int join_find_head(int64_t k, const unsigned long long* slots,
                                const join_sp* sp, int64_t cap_mask) {
  if ((unsigned long long)k == AGG_EMPTY) return sp->m1_head;
  uint64_t slot = join_slot(k, cap_mask);
  for (;;) {
    unsigned long long cur = slots[2 * slot];
    if (cur == AGG_EMPTY) return JOIN_NIL;
    if (cur == (unsigned long long)k) return (unsigned int)slots[2 * slot + 1];
    slot = (slot + 1) & (uint64_t)cap_mask;
  }
}

template <int JT>
__global__ __launch_bounds__(JOIN_BLOCK)
void k_join_probe(int64_t n, const int64_t* keys, const uint8_t* kvalid,
                  const unsigned long long* slots, const unsigned int* next,
                  join_sp* sp, int64_t cap_mask,
                  uint32_t* out_p, uint32_t* out_b, int64_t out_cap,
                  unsigned long long* matched) {
  constexpr int ROUNDS = JOIN_CHUNK / JOIN_BLOCK;
  const int64_t base = (int64_t)blockIdx.x * JOIN_CHUNK + threadIdx.x;
  const join_accept_all accept;
  uint32_t cnt[ROUNDS];
  unsigned int c0[ROUNDS], c1[ROUNDS];
  uint32_t lane_total = 0;
  for (int r = 0; r < ROUNDS; r++) {
    const int64_t i = base + r * JOIN_BLOCK;
    const bool valid = i < n && bit_valid(kvalid, i);
    const unsigned int head =
        valid ? join_find_head(keys[i], slots, sp, cap_mask) : JOIN_NIL;
    join_collect<JT>(head, i, next, matched, accept, &cnt[r], &c0[r], &c1[r]);
    if (JT == 5 && i < n && !valid)
      cnt[r] = 1;  /* null-aware anti: NULL NOT IN (non-empty) is unknown
                    * -> the row is filtered (treated as matched);
                    * BroadcastHashJoinExec.scala:137 NAAJ semantics */
    if (JT == 0) lane_total += cnt[r];
    else if (i < n) lane_total += jt_emit_count(JT, cnt[r]);
  }
  int64_t o = join_reserve(lane_total, &sp->cursor);
  for (int r = 0; r < ROUNDS; r++) {
    const int64_t i = base + r * JOIN_BLOCK;
    join_emit_row<JT>(i, i < n, cnt[r], c0[r], c1[r], next, accept, o,
                      out_p, out_b, out_cap);
  }
}

/* FullOuter second half: one (NIL, build_rid) pair per unmatched build
 * row — every build row never touched by a probe (incl. NULL-key build
 * rows, which are never inserted and so never matched). */
__global__ void k_join_unmatched_build(int64_t brows,
                                       const unsigned long long* matched,
                                       join_sp* sp,
                                       uint32_t* out_p, uint32_t* out_b,
                                       int64_t out_cap) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & (WAVE - 1);
  for (; i - lane < brows; i += gs) {
    bool un = i < brows && !((matched[i >> 6] >> (i & 63)) & 1);
    uint64_t m = __ballot(un);
    if (!m) continue;
    int cntw = __popcll(m);
    unsigned long long base = 0;
    int leader = __ffsll((unsigned long long)m) - 1;
    if (lane == leader)
      base = atomicAdd(&sp->cursor, (unsigned long long)cntw);
    base = __shfl(base, leader);
    if (!un) continue;
    int64_t o = (int64_t)base + __popcll(m & ((1ULL << lane) - 1));
    if (o < out_cap) {
      out_p[o] = JOIN_NIL;
      out_b[o] = (unsigned int)i;
    }
  }
}

/* Host side of every probe: reset the output cursor and, if there are probe
 * rows, launch the kernel instantiation for join_type (which the caller has
 * checked against 0..MAX_JT) as launch(std::integral_constant<int, JT>()). */
template <int MAX_JT, class Launch>
static int join_launch_probe(hipStream_t s, join_sp* sp, int64_t prows,
                             int32_t join_type, const char* tag, Launch launch) {
  HIP_TRY(hipMemsetAsync(&sp->cursor, 0, 8, s));
  if (prows <= 0) return GPUQ_OK;
  hipEvent_t _pe = prof_begin(s);
  switch (join_type) {
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    case 3: launch(std::integral_constant<int, 3>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 5:
      if constexpr (MAX_JT >= 5) launch(std::integral_constant<int, 5>());
      break;
    default: launch(std::integral_constant<int, 0>()); break;
  }
  prof_end(tag, s, _pe);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* read the output cursor back; a count above out_cap is an error the caller
 * answers with a larger buffer */
static int join_read_count(hipStream_t s, const join_sp* sp, const char* who,
                           const char* what, int64_t out_cap, int64_t* out_n) {
  unsigned long long cursor;
  HIP_TRY(hipMemcpyAsync(&cursor, &sp->cursor, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out_n = (int64_t)cursor;
  if ((int64_t)cursor > out_cap)
    FAIL(GPUQ_ERR_OVERFLOW, "%s: %lld %s exceed out_cap %lld", who,
         (long long)cursor, what, (long long)out_cap);
  return GPUQ_OK;
}

extern "C" int gpuq_join_build_i64(void* stream, int64_t brows, gpuq_col bkey,
                                   void* workspace, int64_t cap) {
  hipStream_t s = (hipStream_t)stream;
  if (cap <= 0 || (cap & (cap - 1)))
    FAIL(GPUQ_ERR_INVALID, "join: capacity %lld not a power of two", (long long)cap);
  if (brows > 0x7FFFFFFELL) FAIL(GPUQ_ERR_INVALID, "join: build side too large for 31-bit rowids");
  if (bkey.dtype != GPUQ_INT64) FAIL(GPUQ_ERR_INVALID, "join: key must be int64");
  join_ws w; int64_t need;
  join_ws_layout(cap, brows, &w, (char*)workspace, &need);
  HIP_TRY(hipMemsetAsync(w.slots, 0xFF, cap * 16, s));  /* keys=-1, heads=NIL */
  HIP_TRY(hipMemsetAsync(w.matched, 0, ((brows + 63) / 64) * 8, s));
  HIP_TRY(hipMemsetAsync(w.sp, 0xFF, 4, s));            /* m1_head = NIL */
  HIP_TRY(hipMemsetAsync(&w.sp->cursor, 0, 8, s));
  if (brows == 0) return GPUQ_OK;
  int64_t nchunks = (brows + JOIN_CHUNK - 1) / JOIN_CHUNK;
  { hipEvent_t _pe = prof_begin(s);
  k_join_build<<<dim3((uint32_t)nchunks), 256, 0, s>>>(
      brows, (const int64_t*)bkey.data, bkey.validity, w.slots, w.next, w.sp,
      cap - 1);
  prof_end("join_build", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* probe_workspace / probe_ws_bytes are accepted and ignored (ABI) */
extern "C" int gpuq_join_probe_i64_typed(void* stream, int64_t prows, gpuq_col pkey,
                                   const void* workspace, int64_t cap, int64_t brows,
                                   void* probe_workspace, int64_t probe_ws_bytes,
                                   int32_t join_type,
                                   uint32_t* out_p, uint32_t* out_b,
                                   int64_t out_cap, int64_t* out_nmatches) {
  hipStream_t s = (hipStream_t)stream;
  (void)probe_workspace; (void)probe_ws_bytes;
  if (join_type < 0 || join_type > 5)
    FAIL(GPUQ_ERR_INVALID, "join: bad join_type %d", join_type);
  if (pkey.dtype != GPUQ_INT64) FAIL(GPUQ_ERR_INVALID, "join: key must be int64");
  join_ws w; int64_t need;
  join_ws_layout(cap, brows, &w, (char*)workspace, &need);
  dim3 jg((uint32_t)((prows + JOIN_CHUNK - 1) / JOIN_CHUNK));
  if (int rc = join_launch_probe<5>(s, w.sp, prows, join_type, "join_probe", [&](auto jt) {
        k_join_probe<decltype(jt)::value><<<jg, JOIN_BLOCK, 0, s>>>(
            prows, (const int64_t*)pkey.data, pkey.validity, w.slots, w.next,
            w.sp, cap - 1, out_p, out_b, out_cap, w.matched);
      })) return rc;
  if (join_type == 4 && brows > 0) {
    /* FullOuter second half; probes with zero rows still emit every
     * build row */
    k_join_unmatched_build<<<grid1d(brows), 256, 0, s>>>(
        brows, w.matched, w.sp, out_p, out_b, out_cap);
    HIP_TRY(hipGetLastError());
  }
  return join_read_count(s, w.sp, "join", "matches", out_cap, out_nmatches);
}

extern "C" int gpuq_join_probe_i64(void* stream, int64_t prows, gpuq_col pkey,
                                   const void* workspace, int64_t cap, int64_t brows,
                                   void* probe_workspace, int64_t probe_ws_bytes,
                                   uint32_t* out_p, uint32_t* out_b,
                                   int64_t out_cap, int64_t* out_nmatches) {
  return gpuq_join_probe_i64_typed(stream, prows, pkey, workspace, cap, brows,
                                   probe_workspace, probe_ws_bytes, 0,
                                   out_p, out_b, out_cap, out_nmatches);
}

/* ============ composite-key hash join (multi-column equi-join) ============ */
/*
 * Equi-join on a key tuple (k1..kK), K <= 4 int64 columns with independent
 * NULLability — HashJoin.scala joins on leftKeys/rightKeys: Seq[Expression];
 * the single-long LongHashedRelation above is its special case.
 *
 * One open-address slot per DISTINCT tuple, the tuple stored in the slot:
 *   { u64 sig; u32 head; u32 pad; i64 key[K] }
 * with the stride rounded up to 32 B (K <= 2) or 64 B (K 3-4), so a slot
 * never straddles a 64 B line: random probes pay per line touched, not per
 * byte (profiles/round2_pmc_fetch.txt), and a probe that finds its tuple has
 * touched exactly one. Duplicates chain through next[] off the slot's head
 * word exactly as in the single-key join (join_push_head, JOIN_MULTI,
 * JOIN_NIL).
 *
 * Hashing is the composite aggregate's scheme: slot index from the
 * seed-chained Murmur3 over the tuple, 64-bit signature from a splitmix
 * chain, EMPTY/PENDING reserved signature values real signatures are
 * remapped away from — no special slots, -1 / 0 / INT64_MIN are ordinary
 * key values. Build claims a slot with CAS(sig: EMPTY->PENDING), stores the
 * tuple, then publishes the signature (see k_joink_build for the ordering);
 * a signature hit is verified against the stored tuple, so signature
 * collisions cost probes, never correctness.
 * A row with a NULL in ANY key column is never inserted and never matches
 * (equi-join keys; null-safe <=> is not supported).
 */

#define JOINK_MAX_KEYS 4
#define JOINK_EMPTY 0ULL
#define JOINK_PENDING 1ULL
#define JOINK_SPIN_LIMIT (1u << 22)
#define JOINK_HEAD_INIT 0x00000000FFFFFFFFULL   /* head = JOIN_NIL, pad = 0 */

struct joink_cols { const int64_t* k[JOINK_MAX_KEYS]; const uint8_t* v[JOINK_MAX_KEYS]; };

/* j.cursor: output reservation (shared with k_join_unmatched_build);
 * overflow: 1 = table full, 2 = a PENDING slot was never published */
struct joink_sp { join_sp j; unsigned long long overflow; };

/* slot stride in u64 words: 32 B for K <= 2, 64 B for K 3-4 */
static int joink_stride_words(int nkeys) { return nkeys <= 2 ? 4 : 8; }

struct joink_ws {
  unsigned long long* slots;   /* cap slots of joink_stride_words() u64 */
  unsigned int* next;
  unsigned long long* matched; /* build-row matched bits (full outer) */
  joink_sp* sp;
};

/* pure arithmetic (no device query): argument validation and the CPU tests
 * run without a GPU. slots come first, so they inherit the workspace's
 * alignment (>= 64 B from any device allocator). */
static void joink_ws_layout(int64_t cap, int64_t brows, int nkeys, joink_ws* w,
                            char* base, int64_t* total) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->slots = (unsigned long long*)take(cap * 8 * joink_stride_words(nkeys));
  w->next = (unsigned int*)take(brows * 4);
  w->matched = (unsigned long long*)take(((brows + 63) / 64) * 8);
  w->sp = (joink_sp*)take(sizeof(joink_sp));
  *total = off;
}

extern "C" int64_t gpuq_join_keys_workspace_bytes(int64_t brows, int64_t cap,
                                                  int32_t nkeys) {
  if (brows < 0 || cap <= 0 || nkeys < 1 || nkeys > JOINK_MAX_KEYS) return 0;
  joink_ws w; int64_t total;
  joink_ws_layout(cap, brows, nkeys, &w, nullptr, &total);
  return total;
}

/* shared argument checks; all of them run before any HIP call */
static int joink_check_table(const char* who, int32_t nkeys, int64_t cap,
                             int64_t brows) {
  if (nkeys < 1 || nkeys > JOINK_MAX_KEYS)
    FAIL(GPUQ_ERR_INVALID, "%s: nkeys %d not in [1,%d]", who, nkeys, JOINK_MAX_KEYS);
  if (cap <= 0 || (cap & (cap - 1)))
    FAIL(GPUQ_ERR_INVALID, "%s: capacity %lld not a power of two", who, (long long)cap);
  if (brows < 0 || brows > 0x7FFFFFFELL)
    FAIL(GPUQ_ERR_INVALID, "%s: build rows %lld do not fit 31-bit rowids", who,
         (long long)brows);
  return GPUQ_OK;
}

static int joink_check_cols(const char* who, const gpuq_col* cols, int32_t nkeys,
                            joink_cols* kc) {
  if (!cols) FAIL(GPUQ_ERR_INVALID, "%s: key columns missing", who);
  for (int c = 0; c < nkeys; c++) {
    if (cols[c].dtype != GPUQ_INT64)
      FAIL(GPUQ_ERR_INVALID, "%s: key col %d must be int64", who, c);
    kc->k[c] = (const int64_t*)cols[c].data;
    kc->v[c] = cols[c].validity;
  }
  return GPUQ_OK;
}

/* row i's tuple, slot hash and signature; false if any key column is NULL */
DEV bool joink_load(const joink_cols& kc, int nkeys, int64_t i, int64_t* key,
                    uint32_t* slot_hash, unsigned long long* sig) {
  uint32_t h = 42;
  uint64_t s = 0x243F6A8885A308D3ULL;
#pragma unroll
  for (int c = 0; c < JOINK_MAX_KEYS; c++) {
    if (c < nkeys) {
      if (!bit_valid(kc.v[c], i)) return false;
      int64_t k = kc.k[c][i];
      key[c] = k;
      h = (uint32_t)mm3_hash_long(k, (int32_t)h);
      s = splitmix64((s ^ (uint64_t)k) + (uint64_t)c);
    }
  }
  if (s == JOINK_EMPTY || s == JOINK_PENDING) s = 2;
  *slot_hash = h; *sig = s;
  return true;
}

__global__ void k_joink_init(int64_t cap, int sw, unsigned long long* slots,
                             joink_sp* sp) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < cap; i += gs) {
    slots[i * sw] = JOINK_EMPTY;
    slots[i * sw + 1] = JOINK_HEAD_INIT;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sp->j.m1_head = JOIN_NIL; sp->j.cursor = 0;
    sp->overflow = 0;
  }
}

/* Claim/publish as in k_aggk_build: one attempt per loop iteration, so a
 * lane spinning on PENDING never starves the publisher in its own wave (the
 * publisher's branch runs between iterations). Unlike the aggregate the
 * whole loop is bounded: `cap` slot visits without a home means the table
 * is full, JOINK_SPIN_LIMIT reloads of one PENDING word means its publisher
 * is gone — both set the overflow word and give up.
 * Publication without a per-claim L2 write-back: the tuple words are stored
 * with agent-scope atomics (write-through), the storing lane's wave drains
 * them (vmcnt(0)) and only then stores the signature, also agent-scope; a
 * reader polls the signature relaxed and, on a hit, takes ONE agent acquire
 * before loading the tuple with agent-scope atomic loads. A release on the
 * signature store instead (buffer_wbl2 per claimed slot, plus an L1
 * invalidate per poll from acquire loads) measured 20x the single-key
 * build at 2M distinct tuples (profiles/README.md). */
__global__ __launch_bounds__(256)
void k_joink_build(int64_t n, joink_cols kc, int nkeys, int sw,
                   unsigned long long* slots, unsigned int* next,
                   joink_sp* sp, int64_t cap_mask) {
  int64_t base = (int64_t)blockIdx.x * JOIN_CHUNK;
  for (int r = 0; r < JOIN_CHUNK / 256; r++) {
    int64_t i = base + r * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t key[JOINK_MAX_KEYS];
    uint32_t h; unsigned long long mysig;
    if (!joink_load(kc, nkeys, i, key, &h, &mysig)) continue;  /* NULL never matches */
    uint64_t slot = h & (uint64_t)cap_mask;
    int64_t visits = 0;
    uint32_t spins = 0;
    unsigned long long* sl;
    for (;;) {
      sl = slots + slot * sw;
      unsigned long long cur = __hip_atomic_load(sl, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
      if (cur == JOINK_EMPTY) {
        unsigned long long prev = atomicCAS(sl, JOINK_EMPTY, JOINK_PENDING);
        if (prev == JOINK_EMPTY) {
#pragma unroll
          for (int c = 0; c < JOINK_MAX_KEYS; c++)
            if (c < nkeys)
              __hip_atomic_store(&sl[2 + c], (unsigned long long)key[c],
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          /* drain the write-through tuple stores, then publish */
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(sl, mysig, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        cur = JOINK_PENDING;  /* lost the claim: the word is PENDING or a sig now */
      }
      if (cur == JOINK_PENDING) {
        if (++spins > JOINK_SPIN_LIMIT) { atomicMax(&sp->overflow, 2ull); return; }
        continue;  /* publisher runs between iterations */
      }
      if (cur == mysig) {
        /* acquire only on a signature hit, never per poll */
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        bool eq = true;
#pragma unroll
        for (int c = 0; c < JOINK_MAX_KEYS; c++)
          if (c < nkeys)
            eq = eq && __hip_atomic_load(&sl[2 + c], __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT) ==
                           (unsigned long long)key[c];
        if (eq) break;
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
      if (++visits > cap_mask) { atomicMax(&sp->overflow, 1ull); return; }
    }
    join_push_head((unsigned int*)(sl + 1), (unsigned int)i, next);
  }
}

/* composite-key lookup: the slot walk. A row with a NULL in any key column
 * has no chain. The table was published by an earlier launch, so plain
 * loads suffice. */
DEV unsigned int joink_find_head(const joink_cols& kc, int nkeys, int sw,
                                 const unsigned long long* slots,
                                 int64_t cap_mask, int64_t i) {
  unsigned int head = JOIN_NIL;
  int64_t key[JOINK_MAX_KEYS];
  uint32_t h; unsigned long long mysig;
  if (joink_load(kc, nkeys, i, key, &h, &mysig)) {
    uint64_t slot = h & (uint64_t)cap_mask;
    /* bounded like the build: a (contract-violating) full table ends the
     * walk after cap visits instead of circling */
    for (int64_t visits = 0; visits <= cap_mask; visits++) {
      const unsigned long long* sl = slots + slot * sw;
      unsigned long long cur = sl[0];
      if (cur == JOINK_EMPTY) break;
      if (cur == mysig) {
        bool eq = true;
#pragma unroll
        for (int c = 0; c < JOINK_MAX_KEYS; c++)
          if (c < nkeys) eq = eq && sl[2 + c] == (unsigned long long)key[c];
        if (eq) { head = (unsigned int)sl[1]; break; }
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
    }
  }
  return head;
}

/* The probe skeleton over the composite table; JT 0-4. */
template <int JT>
__global__ __launch_bounds__(JOIN_BLOCK)
void k_joink_probe(int64_t n, joink_cols kc, int nkeys, int sw,
                   const unsigned long long* slots, const unsigned int* next,
                   joink_sp* sp, int64_t cap_mask,
                   uint32_t* out_p, uint32_t* out_b, int64_t out_cap,
                   unsigned long long* matched) {
  constexpr int ROUNDS = JOIN_CHUNK / JOIN_BLOCK;
  const int64_t base = (int64_t)blockIdx.x * JOIN_CHUNK + threadIdx.x;
  const join_accept_all accept;
  uint32_t cnt[ROUNDS];
  unsigned int c0[ROUNDS], c1[ROUNDS];
  uint32_t lane_total = 0;
  for (int r = 0; r < ROUNDS; r++) {
    const int64_t i = base + r * JOIN_BLOCK;
    const unsigned int head =
        i < n ? joink_find_head(kc, nkeys, sw, slots, cap_mask, i) : JOIN_NIL;
    join_collect<JT>(head, i, next, matched, accept, &cnt[r], &c0[r], &c1[r]);
    if (JT == 0) lane_total += cnt[r];
    else if (i < n) lane_total += jt_emit_count(JT, cnt[r]);
  }
  int64_t o = join_reserve(lane_total, &sp->j.cursor);
  for (int r = 0; r < ROUNDS; r++) {
    const int64_t i = base + r * JOIN_BLOCK;
    join_emit_row<JT>(i, i < n, cnt[r], c0[r], c1[r], next, accept, o,
                      out_p, out_b, out_cap);
  }
}

extern "C" int gpuq_join_build_keys(void* stream, int64_t brows,
                                    const gpuq_col* build_keys, int32_t nkeys,
                                    void* workspace, int64_t cap) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = joink_check_table("join_keys build", nkeys, cap, brows)) return rc;
  joink_cols kc = {};
  if (int rc = joink_check_cols("join_keys build", build_keys, nkeys, &kc)) return rc;
  joink_ws w; int64_t need;
  joink_ws_layout(cap, brows, nkeys, &w, (char*)workspace, &need);
  int sw = joink_stride_words(nkeys);
  k_joink_init<<<grid1d(cap), 256, 0, s>>>(cap, sw, w.slots, w.sp);
  HIP_TRY(hipGetLastError());
  if (brows == 0) return GPUQ_OK;
  HIP_TRY(hipMemsetAsync(w.matched, 0, ((brows + 63) / 64) * 8, s));
  int64_t nchunks = (brows + JOIN_CHUNK - 1) / JOIN_CHUNK;
  { hipEvent_t _pe = prof_begin(s);
  k_joink_build<<<dim3((uint32_t)nchunks), 256, 0, s>>>(
      brows, kc, nkeys, sw, w.slots, w.next, w.sp, cap - 1);
  prof_end("join_keys_build", s, _pe); }
  HIP_TRY(hipGetLastError());
  joink_sp hsp;
  HIP_TRY(hipMemcpyAsync(&hsp, w.sp, sizeof(hsp), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (hsp.overflow == 1)
    FAIL(GPUQ_ERR_OVERFLOW, "join_keys build: hash table overflow (capacity %lld)",
         (long long)cap);
  if (hsp.overflow)
    FAIL(GPUQ_ERR_OVERFLOW, "join_keys build: gave up on an unpublished slot "
         "(capacity %lld)", (long long)cap);
  return GPUQ_OK;
}

extern "C" int gpuq_join_probe_keys(void* stream, int64_t prows,
                                    const gpuq_col* probe_keys, int32_t nkeys,
                                    void* workspace, int64_t cap, int64_t brows,
                                    int32_t join_type,
                                    uint32_t* out_p, uint32_t* out_b,
                                    int64_t out_cap, int64_t* out_nmatches) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = joink_check_table("join_keys probe", nkeys, cap, brows)) return rc;
  if (join_type == 5)
    FAIL(GPUQ_ERR_INVALID, "join_keys probe: the null-aware anti join (type 5) "
         "is single-key only");
  if (join_type < 0 || join_type > 4)
    FAIL(GPUQ_ERR_INVALID, "join_keys probe: bad join_type %d", join_type);
  if (prows < 0 || prows > 0xFFFFFFFELL)
    FAIL(GPUQ_ERR_INVALID, "join_keys probe: probe rows %lld do not fit 32-bit rowids",
         (long long)prows);
  joink_cols kc = {};
  if (int rc = joink_check_cols("join_keys probe", probe_keys, nkeys, &kc)) return rc;
  joink_ws w; int64_t need;
  joink_ws_layout(cap, brows, nkeys, &w, (char*)workspace, &need);
  int sw = joink_stride_words(nkeys);
  dim3 jg((uint32_t)((prows + JOIN_CHUNK - 1) / JOIN_CHUNK));
  if (int rc = join_launch_probe<4>(s, &w.sp->j, prows, join_type, "join_keys_probe", [&](auto jt) {
        k_joink_probe<decltype(jt)::value><<<jg, JOIN_BLOCK, 0, s>>>(
            prows, kc, nkeys, sw, w.slots, w.next, w.sp, cap - 1, out_p, out_b,
            out_cap, w.matched);
      })) return rc;
  return join_read_count(s, &w.sp->j, "join_keys probe", "matches", out_cap,
                         out_nmatches);
}

extern "C" int gpuq_join_keys_unmatched_build(void* stream, void* workspace,
                                              int64_t cap, int64_t brows,
                                              int32_t nkeys,
                                              uint32_t* out_p, uint32_t* out_b,
                                              int64_t out_cap, int64_t* out_nrows) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = joink_check_table("join_keys unmatched", nkeys, cap, brows)) return rc;
  joink_ws w; int64_t need;
  joink_ws_layout(cap, brows, nkeys, &w, (char*)workspace, &need);
  HIP_TRY(hipMemsetAsync(&w.sp->j.cursor, 0, 8, s));
  if (brows > 0) {
    k_join_unmatched_build<<<grid1d(brows), 256, 0, s>>>(
        brows, w.matched, &w.sp->j, out_p, out_b, out_cap);
    HIP_TRY(hipGetLastError());
  }
  return join_read_count(s, &w.sp->j, "join_keys unmatched", "rows", out_cap,
                         out_nrows);
}

/* ---- partitioned aggregation (mid/high cardinality) ----
 * The direct table is atomic-throughput-bound (~22 G f64-adds/s at 10M
 * groups, tools/diag_hash.py). Round-2 design: ONE non-stable 13-bit
 * bucket partition (8192 buckets; aggregation does not need stability, so
 * the two 16-bit ranked-scatter passes of round 1 — 2x the scatter
 * kernel's internal ceiling — are replaced by a histogram + reserve +
 * direct scatter whose per-block per-bucket runs are ~0.5 KB contiguous
 * stores), then per-chunk LDS-table aggregation: a 16 K-row chunk of
 * bucket-ordered data holds at most ~n_groups/8192 (+ one bucket boundary)
 * distinct keys, and a chunk that ever overflows the LDS table flushes it
 * to the global table mid-chunk and continues (skew-safe, no global
 * fallback). */

#define PAGG_BUCKETS_MAX 16384
#define PAGG_TILE (256 * 1024)    /* rows partitioned per block */

template <int BUCKETS>
DEV int pagg_bucket(int64_t k) {
  /* top bits below the sign of the 32-bit murmur */
  return (int)(((uint32_t)mm3_hash_long(k, 42) >> 12) & (BUCKETS - 1));
}

/* global bucket histogram; NULL-key rows count via key 0, real -1 keys via
 * their own hash — the scatter uses identical bucketing and marks those
 * records EMPTY, so layout and content agree. */
template <int BUCKETS>
__global__ void k_pagg_ghist(int64_t n, const int64_t* keys, const uint8_t* kvalid,
                             unsigned int* ghist) {
  __shared__ unsigned int h[BUCKETS];
  for (int b = threadIdx.x; b < BUCKETS; b += blockDim.x) h[b] = 0;
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) {
    int64_t k = bit_valid(kvalid, i) ? keys[i] : 0;
    atomicAdd(&h[pagg_bucket<BUCKETS>(k)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < BUCKETS; b += blockDim.x)
    if (h[b]) atomicAdd(&ghist[b], h[b]);
}

/* single-block exclusive scan of the bucket histogram -> running cursors */
template <int BUCKETS>
__global__ void k_pagg_scan(const unsigned int* ghist, unsigned int* gcursor) {
  __shared__ unsigned int buf[BUCKETS];
  for (int b = threadIdx.x; b < BUCKETS; b += blockDim.x)
    buf[b] = ghist[b];
  __syncthreads();
  if (threadIdx.x == 0) {           /* serial adds, once per aggregate call */
    unsigned int run = 0;
    for (int b = 0; b < BUCKETS; b++) {
      unsigned int t = buf[b];
      buf[b] = run;
      run += t;
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < BUCKETS; b += blockDim.x)
    gcursor[b] = buf[b];
}

/* bucket scatter: per block, histogram its tile, reserve per-bucket ranges
 * with ONE global atomicAdd per (block, bucket), then write (key, val)
 * records bucket-contiguously. Special rows (NULL key / key == -1 ==
 * AGG_EMPTY) accumulate into the special slots and leave EMPTY records. */
template <int OPS, int BUCKETS, int SBLOCK, int ST /*0 plain,1 sc1,2 nt*/>
__global__ __launch_bounds__(SBLOCK)
void k_pagg_scatter(int64_t n, const int64_t* keys, const uint8_t* kvalid,
                    const double* vals, unsigned int* gcursor,
                    ulonglong2* recs, agg_special* sp) {
  __shared__ unsigned int h[BUCKETS];
  __shared__ unsigned int base[BUCKETS];
  const int64_t t0 = (int64_t)blockIdx.x * PAGG_TILE;
  const int64_t t1 = min(t0 + (int64_t)PAGG_TILE, n);
  for (int b = threadIdx.x; b < BUCKETS; b += blockDim.x) h[b] = 0;
  __syncthreads();
  for (int64_t i = t0 + threadIdx.x; i < t1; i += blockDim.x) {
    int64_t k = bit_valid(kvalid, i) ? keys[i] : 0;
    atomicAdd(&h[pagg_bucket<BUCKETS>(k)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < BUCKETS; b += blockDim.x)
    base[b] = h[b] ? atomicAdd(&gcursor[b], h[b]) : 0u;
  __syncthreads();
  for (int64_t i = t0 + threadIdx.x; i < t1; i += blockDim.x) {
    bool kv = bit_valid(kvalid, i);
    int64_t k = kv ? keys[i] : 0;
    double v = vals[i];
    unsigned int pos = atomicAdd(&base[pagg_bucket<BUCKETS>(k)], 1u);
    ulonglong2 rec;
    if (!kv || (unsigned long long)k == AGG_EMPTY) {
      unsigned long long* pseen = kv ? &sp->m1_seen : &sp->nul_seen;
      double* psum = kv ? &sp->m1_sum : &sp->nul_sum;
      unsigned long long* pcnt = kv ? &sp->m1_cnt : &sp->nul_cnt;
      atomicMax(pseen, 1ull);
      if (OPS & AGG_OP_SUM) atomicAdd(psum, v);
      if (OPS & AGG_OP_COUNT) atomicAdd(pcnt, 1ull);
      rec.x = AGG_EMPTY;
      rec.y = 0;
    } else {
      rec.x = (unsigned long long)k;
      rec.y = (unsigned long long)__double_as_longlong(v);
    }
    if (ST == 1) {
      /* write-through: the per-bucket runs are written temporally
       * scattered across the tile scan, so cached lines rarely collect a
       * full 64 B before eviction — skip the write-allocate RFO */
      __hip_atomic_store(&recs[pos].x, rec.x, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&recs[pos].y, rec.y, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    } else if (ST == 2) {
      __builtin_nontemporal_store(rec.x, &recs[pos].x);
      __builtin_nontemporal_store(rec.y, &recs[pos].y);
    } else {
      recs[pos] = rec;
    }
  }
}

/* chunk aggregation over bucket-ordered records with mid-chunk flush: when
 * any thread cannot place its key (LDS table full — a skewed or
 * boundary-spanning chunk), the whole block merges the table into the
 * global one, clears it, and the failed inserts retry. */
template <int OPS, int SLOT, int SLOTS, int CHUNK, int CBLOCK>
__global__ __launch_bounds__(CBLOCK)
void k_agg_part(int64_t n, const ulonglong2* recs,
                unsigned long long* tab, agg_special* sp, int64_t cap_mask) {
  __shared__ unsigned long long lt[SLOTS * 3];
  const int64_t base = (int64_t)blockIdx.x * CHUNK;
  for (int j = threadIdx.x; j < SLOTS * 3; j += blockDim.x)
    lt[j] = (j % 3 == 0) ? AGG_EMPTY : 0;
  __syncthreads();
  auto merge_flush = [&]() {
    for (int j = threadIdx.x; j < SLOTS; j += blockDim.x) {
      unsigned long long k = lt[3 * j];
      if (k == AGG_EMPTY) continue;
      uint64_t slot = ((uint32_t)mm3_hash_long((int64_t)k, 42)) & (uint64_t)cap_mask;
      for (int64_t probes = 0;; probes++) {
        unsigned long long cur = __hip_atomic_load(&tab[SLOT * slot], __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        if (cur == k) break;
        if (cur == AGG_EMPTY) {
          unsigned long long prev = atomicCAS(&tab[SLOT * slot], AGG_EMPTY, k);
          if (prev == AGG_EMPTY || prev == k) break;
        }
        slot = (slot + 1) & (uint64_t)cap_mask;
        if (probes > cap_mask) { atomicMax(&sp->overflow, 1ull); return; }
      }
      if (OPS & AGG_OP_SUM)
        atomicAdd((double*)&tab[SLOT * slot + 1],
                  __longlong_as_double((long long)lt[3 * j + 1]));
      if (OPS & AGG_OP_COUNT) atomicAdd(&tab[SLOT * slot + 2], lt[3 * j + 2]);
    }
  };
  static_assert((CHUNK / CBLOCK) % 4 == 0, "round grouping");
  for (int r0 = 0; r0 < CHUNK / CBLOCK; r0 += 4) {
    /* batch 4 record loads in flight before the dependent hash->LDS-probe
     * chain (the LDS table path is latency-, not queue-bound) */
    ulonglong2 recv[4];
    bool havev[4];
    #pragma unroll
    for (int q = 0; q < 4; q++) {
      int64_t i = base + (int64_t)(r0 + q) * CBLOCK + threadIdx.x;
      havev[q] = i < n;
      if (havev[q]) recv[q] = recs[i];
    }
    #pragma unroll
    for (int q = 0; q < 4; q++)
      havev[q] = havev[q] && recv[q].x != AGG_EMPTY;
    for (int q = 0; q < 4; q++) {
    ulonglong2 rec = recv[q];
    bool have = havev[q];
    for (;;) {
      bool fail = false;
      if (have) {
        uint64_t slot = ((uint32_t)mm3_hash_long((int64_t)rec.x, 42)) &
                        (SLOTS - 1);
        int probes = 0;
        for (;; probes++) {
          unsigned long long cur = lt[3 * slot];
          if (cur == rec.x) break;
          if (cur == AGG_EMPTY) {
            unsigned long long prev = atomicCAS(&lt[3 * slot], AGG_EMPTY, rec.x);
            if (prev == AGG_EMPTY || prev == rec.x) break;
          }
          slot = (slot + 1) & (SLOTS - 1);
          if (probes >= SLOTS) { fail = true; break; }
        }
        if (!fail) {
          if (OPS & AGG_OP_SUM)
            atomicAdd((double*)&lt[3 * slot + 1],
                      __longlong_as_double((long long)rec.y));
          if (OPS & AGG_OP_COUNT) atomicAdd(&lt[3 * slot + 2], 1ull);
          have = false;
        }
      }
      if (__syncthreads_count(fail ? 1 : 0) == 0) break;
      merge_flush();
      __syncthreads();
      for (int j = threadIdx.x; j < SLOTS * 3; j += blockDim.x)
        lt[j] = (j % 3 == 0) ? AGG_EMPTY : 0;
      __syncthreads();
    }
    }
  }
  __syncthreads();
  merge_flush();
}

struct pagg_ws {
  ulonglong2* recs;
  unsigned int* ghist;
  unsigned int* gcursor;
  unsigned long long* tab;
  agg_special* sp;
};

static void pagg_ws_layout(int64_t n, int64_t cap, pagg_ws* w, char* base, int64_t* total) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->recs = (ulonglong2*)take(n * 16);
  w->ghist = (unsigned int*)take(PAGG_BUCKETS_MAX * 4);
  w->gcursor = (unsigned int*)take(PAGG_BUCKETS_MAX * 4);
  w->tab = (unsigned long long*)take(cap * 24);
  w->sp = (agg_special*)take(sizeof(agg_special));
  *total = off;
}

extern "C" int64_t gpuq_hash_agg_part_workspace_bytes(int64_t n, int64_t cap) {
  pagg_ws w; int64_t total;
  pagg_ws_layout(n, cap, &w, nullptr, &total);
  return total;
}

/* Partitioned aggregation: same results contract as gpuq_hash_agg_i64_f64
 * (single-shot; requires non-null values). */
extern "C" int gpuq_hash_agg_partitioned(void* stream, int64_t n,
                                         gpuq_col key, gpuq_col val,
                                         void* workspace, int64_t cap, int32_t ops,
                                         int64_t* out_keys, uint8_t* out_key_valid,
                                         double* out_sums, uint8_t* out_sum_valid,
                                         int64_t* out_counts, int64_t* out_ngroups) {
  hipStream_t s = (hipStream_t)stream;
  if (cap <= 0 || (cap & (cap - 1)))
    FAIL(GPUQ_ERR_INVALID, "pagg: capacity %lld not a power of two", (long long)cap);
  if (n > 0xFFFFFFFELL)
    FAIL(GPUQ_ERR_INVALID, "pagg: nrows %lld > 2^32 (u32 bucket cursors)", (long long)n);
  if (key.dtype != GPUQ_INT64 || val.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "pagg: expected int64 key + float64 val");
  if (val.validity) FAIL(GPUQ_ERR_INVALID, "pagg: values must be non-null");
  pagg_ws w; int64_t need;
  pagg_ws_layout(n, cap, &w, (char*)workspace, &need);
  k_agg_init<3><<<grid1d(cap), 256, 0, s>>>(cap, w.tab);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(w.sp, 0, sizeof(agg_special), s));
  HIP_TRY(hipMemsetAsync(w.ghist, 0, PAGG_BUCKETS_MAX * 4, s));
  /* variant sweep knob: GPUQ_PAGG=0 (8192 buckets / 2048-slot 16K chunks)
   * 1 (16384 buckets / 4096-slot chunks) 2 (8192 buckets / 4096-slot) */
  static int variant = -1;
  if (variant < 0) {
    const char* e = getenv("GPUQ_PAGG");
    variant = e ? atoi(e) : 2;  /* 8192 buckets / 4096-slot chunks measured best */
  }
  if (n > 0) {
    { hipEvent_t _pe = prof_begin(s);
    if (variant == 1)
      k_pagg_ghist<16384><<<grid1d(n), 256, 0, s>>>(n, (const int64_t*)key.data,
                                                    key.validity, w.ghist);
    else
      k_pagg_ghist<8192><<<grid1d(n), 256, 0, s>>>(n, (const int64_t*)key.data,
                                                   key.validity, w.ghist);
    prof_end("pagg_ghist", s, _pe); }
    HIP_TRY(hipGetLastError());
    if (variant == 1)
      k_pagg_scan<16384><<<1, 256, 0, s>>>(w.ghist, w.gcursor);
    else
      k_pagg_scan<8192><<<1, 256, 0, s>>>(w.ghist, w.gcursor);
    HIP_TRY(hipGetLastError());
    int64_t nblocks = (n + PAGG_TILE - 1) / PAGG_TILE;
    static int st = -1;
    if (st < 0) {
      const char* e = getenv("GPUQ_PAGG_ST");
      st = e ? atoi(e) : 0;  /* plain stores measured best (sc1 +105%, nt +120%) */
    }
    { hipEvent_t _pe = prof_begin(s);
    #define PAGG_LAUNCH(OPS_, B_, T_) do { \
      if (st == 1) k_pagg_scatter<OPS_, B_, T_, 1><<<dim3((uint32_t)nblocks), T_, 0, s>>>( \
          n, (const int64_t*)key.data, key.validity, (const double*)val.data, \
          w.gcursor, w.recs, w.sp); \
      else if (st == 2) k_pagg_scatter<OPS_, B_, T_, 2><<<dim3((uint32_t)nblocks), T_, 0, s>>>( \
          n, (const int64_t*)key.data, key.validity, (const double*)val.data, \
          w.gcursor, w.recs, w.sp); \
      else k_pagg_scatter<OPS_, B_, T_, 0><<<dim3((uint32_t)nblocks), T_, 0, s>>>( \
          n, (const int64_t*)key.data, key.validity, (const double*)val.data, \
          w.gcursor, w.recs, w.sp); \
    } while (0)
    if (variant == 1) {
      if (ops == AGG_OP_SUM) PAGG_LAUNCH(AGG_OP_SUM, 16384, 1024);
      else PAGG_LAUNCH(3, 16384, 1024);
    } else {
      if (ops == AGG_OP_SUM) PAGG_LAUNCH(AGG_OP_SUM, 8192, 512);
      else PAGG_LAUNCH(3, 8192, 512);
    }
    #undef PAGG_LAUNCH
    prof_end("pagg_scatter", s, _pe); }
    HIP_TRY(hipGetLastError());
    { hipEvent_t _pe = prof_begin(s);
    int64_t nchunks = (n + 16384 - 1) / 16384;
    if (variant >= 1) {
      if (ops == AGG_OP_SUM)
        k_agg_part<AGG_OP_SUM, 3, 4096, 16384, 512><<<dim3((uint32_t)nchunks), 512, 0, s>>>(
            n, w.recs, w.tab, w.sp, cap - 1);
      else
        k_agg_part<3, 3, 4096, 16384, 512><<<dim3((uint32_t)nchunks), 512, 0, s>>>(
            n, w.recs, w.tab, w.sp, cap - 1);
    } else {
      if (ops == AGG_OP_SUM)
        k_agg_part<AGG_OP_SUM, 3, 2048, 16384, 256><<<dim3((uint32_t)nchunks), 256, 0, s>>>(
            n, w.recs, w.tab, w.sp, cap - 1);
      else
        k_agg_part<3, 3, 2048, 16384, 256><<<dim3((uint32_t)nchunks), 256, 0, s>>>(
            n, w.recs, w.tab, w.sp, cap - 1);
    }
    prof_end("pagg_chunks", s, _pe); }
    HIP_TRY(hipGetLastError());
  }
  agg_special hsp;
  HIP_TRY(hipMemcpyAsync(&hsp, w.sp, sizeof(hsp), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (hsp.overflow) FAIL(GPUQ_ERR_OVERFLOW, "pagg: table overflow (capacity %lld)", (long long)cap);
  dim3 cgrid((uint32_t)((cap + AGGC_CHUNK - 1) / AGGC_CHUNK));
  if (ops == AGG_OP_SUM)
    k_agg_compact<AGG_OP_SUM, 3><<<cgrid, 256, 0, s>>>(
        cap, w.tab, w.sp, out_keys, out_key_valid, out_sums, out_sum_valid, out_counts);
  else
    k_agg_compact<3, 3><<<cgrid, 256, 0, s>>>(
        cap, w.tab, w.sp, out_keys, out_key_valid, out_sums, out_sum_valid, out_counts);
  HIP_TRY(hipGetLastError());
  agg_special hsp2;
  HIP_TRY(hipMemcpyAsync(&hsp2, w.sp, sizeof(hsp2), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out_ngroups = (int64_t)hsp2.out_cursor;
  return GPUQ_OK;
}

/* ================= multi-aggregate ================= *//* ================= multi-aggregate ================= */
/*
 * One pass computing up to GPUQ_AGG_MAX_SPECS accumulators per group
 * (HashAggregateExec evaluates a LIST of aggregate expressions —
 * HashAggregateExec.scala:68-76; TPC-H Q1 has 8). Slot layout:
 * [key][acc_0]..[acc_{A-1}], stride = 1+A u64 words. SUM accs are f64
 * bits, COUNT accs u64. Small tables (cap*(1+A)*8 <= 64 KB) aggregate in
 * a per-block LDS table first (contention wall removal, same as the
 * single-value path). Round-1 constraint: SUM value columns must be
 * non-null (per-acc NULL tracking pairs a SUM with a COUNT spec).
 */

#define AGG_MAX_SPECS 12

struct agg_cols { const double* p[AGG_MAX_SPECS]; };
/* ops (Sum.scala:113-180, Count.scala, Min/Max.scala null-skipping update
 * expressions): 0=SUM_F64 1=COUNT(col) 2=COUNT(*) 3=SUM_I64(wrapping)
 * 4=MIN_I64 5=MAX_I64 6=MIN_F64 7=MAX_F64. MIN/MAX accumulators hold the
 * monotone u64 encoding (encode_i64/encode_f64) so u64 atomicMin/atomicMax
 * realize the float64 order the sort and the window functions use: NaN
 * greatest and all NaNs equal, -0.0 == 0.0 (encode_f64 folds -0.0 to +0.0
 * and every NaN to the canonical one). The compact pass decodes, so a zero
 * result is +0.0 and a NaN result the canonical NaN. Spark's Double.compare
 * puts -0.0 below 0.0 and would return -0.0 for a group whose extreme is
 * -0.0; here that group returns +0.0. All value ops skip NULL rows; an
 * all-NULL group's acc stays at its init value — callers discriminate via a
 * paired COUNT (Sum/Min/Max evaluate to NULL iff no non-null input).
 * 8=SUM_DEC128 9=DEC128_HI 10=MERGE_DEC128: exact 128-bit SUM of scaled-
 * decimal int64 values (Sum.scala's Decimal path, result
 * decimal(min(38,p+10),s)). The accumulator is TWO adjacent words (lo, hi):
 * op 8/10 owns word j and must be followed by op 9 owning word j+1, so a
 * decimal sum costs two of the AGG_MAX_SPECS slots. Both words init to 0,
 * so strides, init, compaction and emit are untouched. */
struct agg_ops_spec { int op[AGG_MAX_SPECS]; };
struct agg_valid { const uint8_t* v[AGG_MAX_SPECS]; };
struct agg_outs { void* p[AGG_MAX_SPECS]; };

DEV unsigned long long aggm_acc_init(int op) {
  return (op == 4 || op == 6) ? ~0ULL : 0ULL;  /* MIN: u64 max; else 0 */
}

struct agg_multi_special {
  unsigned long long acc[2][AGG_MAX_SPECS];  /* [0]=key -1 group, [1]=NULL group */
  unsigned long long seen[2];
  unsigned long long out_cursor;
  unsigned long long overflow;
};

struct agg_multi_ws {
  unsigned long long* tab;
  agg_multi_special* sp;
};

static void agg_multi_ws_layout(int64_t cap, int nspecs, agg_multi_ws* w,
                                char* base, int64_t* total) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->tab = (unsigned long long*)take(cap * 8 * (1 + nspecs));
  w->sp = (agg_multi_special*)take(sizeof(agg_multi_special));
  *total = off;
}

extern "C" int64_t gpuq_hash_agg_multi_workspace_bytes(int64_t cap, int32_t nspecs) {
  agg_multi_ws w; int64_t total;
  agg_multi_ws_layout(cap, nspecs, &w, nullptr, &total);
  return total;
}

__global__ void k_aggm_init(int64_t cap, int stride, unsigned long long* tab,
                            agg_ops_spec ops, agg_multi_special* sp) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < cap; i += gs) {
    tab[(int64_t)stride * i] = AGG_EMPTY;
    for (int j = 1; j < stride; j++)
      tab[(int64_t)stride * i + j] = aggm_acc_init(ops.op[j - 1]);
  }
  if (sp && blockIdx.x == 0 && threadIdx.x == 0) {
    sp->seen[0] = sp->seen[1] = 0;
    sp->out_cursor = 0;
    sp->overflow = 0;
    for (int w = 0; w < 2; w++)
      for (int j = 0; j < stride - 1; j++) sp->acc[w][j] = aggm_acc_init(ops.op[j]);
  }
}

DEV void aggm_update(unsigned long long* acc, int nspecs, const agg_ops_spec ops,
                     const agg_cols cols, const agg_valid av, int64_t i) {
  for (int j = 0; j < nspecs; j++) {
    int op = ops.op[j];
    if (op == 2) { atomicAdd(&acc[j], 1ull); continue; }  /* COUNT(*) */
    if (!bit_valid(av.v[j], i)) continue;  /* every other op skips NULLs */
    if (op == 0) {
      atomicAdd((double*)&acc[j], cols.p[j][i]);
    } else if (op == 1) {
      atomicAdd(&acc[j], 1ull);
    } else if (op == 3) {
      /* SUM(int64) -> int64 (Sum.scala resultType LongType; non-ansi
       * overflow wraps = two's-complement u64 add, bit-exact) */
      atomicAdd(&acc[j], (unsigned long long)((const int64_t*)cols.p[j])[i]);
    } else if (op == 4 || op == 5) {
      unsigned long long e = encode_i64(((const int64_t*)cols.p[j])[i]);
      if (op == 4) atomicMin(&acc[j], e); else atomicMax(&acc[j], e);
    } else if (op == 8 || op == 10) {
      /* 128-bit two's-complement add into (acc[j], acc[j+1]). op 8 sign-
       * extends an int64 value; op 10 adds a 128-bit partial whose hi word
       * is op 9's column. Every wrap of lo is observed by exactly one
       * returning atomic, which forwards that carry to hi — so the pair is
       * the exact sum in any arrival order, with no CAS loop. */
      unsigned long long add_lo = (unsigned long long)((const int64_t*)cols.p[j])[i];
      unsigned long long add_hi = op == 8
          ? ((long long)add_lo < 0 ? ~0ULL : 0ULL)
          : (unsigned long long)((const int64_t*)cols.p[j + 1])[i];
      unsigned long long old = atomicAdd(&acc[j], add_lo);
      add_hi += (old + add_lo) < old;
      if (add_hi) atomicAdd(&acc[j + 1], add_hi);
    } else if (op == 9) {
      /* DEC128_HI: written by the preceding op 8/10 */
    } else {  /* 6/7: MIN/MAX f64 via the monotone encoding */
      unsigned long long e = encode_f64(cols.p[j][i]);
      if (op == 6) atomicMin(&acc[j], e); else atomicMax(&acc[j], e);
    }
  }
}

/* merge one accumulator word from a sub-table into the global table */
DEV void aggm_merge_acc(unsigned long long* dst, int op, unsigned long long v) {
  if (op == 0)
    atomicAdd((double*)dst, __longlong_as_double((long long)v));
  else if (op == 4 || op == 6) atomicMin(dst, v);
  else if (op == 5 || op == 7) atomicMax(dst, v);
  else if (op == 8 || op == 10) {
    /* dec128 lo word: only the carry out of this add goes to dst[1] here;
     * the sub-table's hi word reaches dst[1] through op 9's own plain add
     * below when the flush loop gets to j+1 — so hi is added exactly once */
    unsigned long long old = atomicAdd(dst, v);
    if ((old + v) < old) atomicAdd(dst + 1, 1ull);
  }
  else atomicAdd(dst, v);  /* COUNT + SUM_I64 + DEC128_HI */
}

template <bool LDS>
__global__ __launch_bounds__(256)
void k_aggm_build(int64_t n, const int64_t* keys, const uint8_t* kvalid,
                  agg_cols cols, agg_ops_spec ops, agg_valid av, int nspecs,
                  unsigned long long* tab, agg_multi_special* sp,
                  int64_t cap_mask) {
  const int stride = 1 + nspecs;
  extern __shared__ __attribute__((aligned(16))) unsigned long long lt[];
  if (LDS) {
    for (int j = threadIdx.x; j < (int)(cap_mask + 1) * stride; j += blockDim.x) {
      int r = j % stride;
      lt[j] = (r == 0) ? AGG_EMPTY : aggm_acc_init(ops.op[r - 1]);
    }
    __syncthreads();
  }
  unsigned long long* t = LDS ? lt : tab;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) {
    bool kv = bit_valid(kvalid, i);
    int64_t k = kv ? keys[i] : 0;
    if (!kv || (unsigned long long)k == AGG_EMPTY) {
      int which = kv ? 0 : 1;
      atomicMax(&sp->seen[which], 1ull);
      aggm_update(sp->acc[which], nspecs, ops, cols, av, i);
      continue;
    }
    uint64_t slot = ((uint32_t)mm3_hash_long(k, 42)) & (uint64_t)cap_mask;
    for (int probes = 0;; probes++) {
      unsigned long long cur = LDS ? t[(int64_t)stride * slot]
          : __hip_atomic_load(&t[(int64_t)stride * slot], __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
      if (cur == (unsigned long long)k) break;
      if (cur == AGG_EMPTY) {
        unsigned long long prev = atomicCAS(&t[(int64_t)stride * slot], AGG_EMPTY,
                                            (unsigned long long)k);
        if (prev == AGG_EMPTY || prev == (unsigned long long)k) break;
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
      if (probes > cap_mask) { atomicMax(&sp->overflow, 1ull); return; }
    }
    aggm_update(&t[(int64_t)stride * slot + 1], nspecs, ops, cols, av, i);
  }
  if (LDS) {
    __syncthreads();
    for (int sI = threadIdx.x; sI < (int)(cap_mask + 1); sI += blockDim.x) {
      unsigned long long k = lt[(int64_t)stride * sI];
      if (k == AGG_EMPTY) continue;
      uint64_t slot = ((uint32_t)mm3_hash_long((int64_t)k, 42)) & (uint64_t)cap_mask;
      /* bounded like the build probe: the global table can fill up with
       * other blocks' keys although no block's own table overflowed */
      bool placed = true;
      for (int64_t probes = 0;; probes++) {
        unsigned long long cur = __hip_atomic_load(&tab[(int64_t)stride * slot],
                                                   __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        if (cur == k) break;
        if (cur == AGG_EMPTY) {
          unsigned long long prev = atomicCAS(&tab[(int64_t)stride * slot], AGG_EMPTY, k);
          if (prev == AGG_EMPTY || prev == k) break;
        }
        slot = (slot + 1) & (uint64_t)cap_mask;
        if (probes > cap_mask) { atomicMax(&sp->overflow, 1ull); placed = false; break; }
      }
      if (!placed) continue;
      for (int j = 0; j < nspecs; j++)
        aggm_merge_acc(&tab[(int64_t)stride * slot + 1 + j], ops.op[j],
                       lt[(int64_t)stride * sI + 1 + j]);
    }
  }
}

DEV void aggm_emit(void* out, int64_t o, int op, unsigned long long v) {
  if (op == 0) ((double*)out)[o] = __longlong_as_double((long long)v);
  else if (op == 4 || op == 5) ((int64_t*)out)[o] = decode_i64(v);
  else if (op == 6 || op == 7) ((double*)out)[o] = decode_f64(v);
  else ((int64_t*)out)[o] = (int64_t)v;
}

__global__ void k_aggm_compact(int64_t cap, const unsigned long long* tab,
                               agg_multi_special* sp, agg_ops_spec ops, int nspecs,
                               int64_t* out_keys, uint8_t* out_kvalid,
                               agg_outs outs) {
  constexpr int ROUNDS = AGGC_CHUNK / 256;
  const int stride = 1 + nspecs;
  __shared__ unsigned long long block_base;
  __shared__ uint32_t wtot[4];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t base = (int64_t)blockIdx.x * AGGC_CHUNK;
  uint32_t occ_mask[ROUNDS / 32 + 1];
  for (int m = 0; m < ROUNDS / 32 + 1; m++) occ_mask[m] = 0;
  uint32_t lane_total = 0;
  for (int r = 0; r < ROUNDS; r++) {
    int64_t i = base + r * 256 + threadIdx.x;
    bool occ = i < cap && tab[(int64_t)stride * i] != AGG_EMPTY;
    if (occ) { occ_mask[r / 32] |= 1u << (r & 31); lane_total++; }
  }
  uint32_t incl = wave_inclusive_scan(lane_total);
  if (lane == WAVE - 1) wtot[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int w = 0; w < 4; w++) { uint32_t t = wtot[w]; wtot[w] = tot; tot += t; }
    block_base = tot ? atomicAdd(&sp->out_cursor, (unsigned long long)tot) : 0;
  }
  __syncthreads();
  int64_t o = (int64_t)block_base + wtot[wave] + (incl - lane_total);
  for (int r = 0; r < ROUNDS; r++) {
    if (!((occ_mask[r / 32] >> (r & 31)) & 1)) continue;
    int64_t i = base + r * 256 + threadIdx.x;
    out_keys[o] = (int64_t)tab[(int64_t)stride * i];
    out_kvalid[o] = 1;
    for (int j = 0; j < nspecs; j++)
      aggm_emit(outs.p[j], o, ops.op[j], tab[(int64_t)stride * i + 1 + j]);
    o++;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int which = 0; which < 2; which++) {
      if (!sp->seen[which]) continue;
      int64_t q = (int64_t)atomicAdd(&sp->out_cursor, 1ull);
      out_keys[q] = which == 0 ? -1 : 0;
      out_kvalid[q] = which == 0 ? 1 : 0;
      for (int j = 0; j < nspecs; j++)
        aggm_emit(outs.p[j], q, ops.op[j], sp->acc[which][j]);
    }
  }
}

/* ops 8/9/10 pairing rule, checked before anything is launched */
static int agg_dec128_check(const char* who, const gpuq_col* vals,
                            const int32_t* spec_ops, const int32_t* spec_cols,
                            int nspecs) {
  for (int j = 0; j < nspecs; j++) {
    int op = spec_ops[j];
    if (op == 8 || op == 10) {
      if (j + 1 >= nspecs || spec_ops[j + 1] != 9)
        FAIL(GPUQ_ERR_INVALID, "%s: dec128 op %d at spec %d must be followed by op 9", who, op, j);
      if (vals[spec_cols[j]].dtype != GPUQ_INT64)
        FAIL(GPUQ_ERR_INVALID, "%s: dec128 op %d needs an int64 column", who, op);
      if (op == 10 && vals[spec_cols[j + 1]].dtype != GPUQ_INT64)
        FAIL(GPUQ_ERR_INVALID, "%s: dec128 partial hi column must be int64", who);
    } else if (op == 9) {
      if (j == 0 || (spec_ops[j - 1] != 8 && spec_ops[j - 1] != 10))
        FAIL(GPUQ_ERR_INVALID, "%s: op 9 at spec %d must follow op 8 or 10", who, j);
    }
  }
  return GPUQ_OK;
}

extern "C" int gpuq_hash_agg_multi(void* stream, int64_t n, gpuq_col key,
                                   const gpuq_col* vals, const int32_t* spec_ops,
                                   const int32_t* spec_cols, int32_t nspecs,
                                   void* workspace, int64_t cap,
                                   int32_t first_batch, int32_t finalize,
                                   int64_t* out_keys, uint8_t* out_key_valid,
                                   void* const* out_accs, int64_t* out_ngroups) {
  hipStream_t s = (hipStream_t)stream;
  if (cap <= 0 || (cap & (cap - 1)))
    FAIL(GPUQ_ERR_INVALID, "aggm: capacity %lld not a power of two", (long long)cap);
  if (nspecs < 1 || nspecs > AGG_MAX_SPECS)
    FAIL(GPUQ_ERR_INVALID, "aggm: nspecs %d not in [1,%d]", nspecs, AGG_MAX_SPECS);
  if (key.dtype != GPUQ_INT64) FAIL(GPUQ_ERR_INVALID, "aggm: key must be int64");
  if (int rc = agg_dec128_check("aggm", vals, spec_ops, spec_cols, nspecs)) return rc;
  agg_cols cols = {}; agg_ops_spec ops = {}; agg_valid av = {};
  for (int j = 0; j < nspecs; j++) {
    int op = spec_ops[j];
    ops.op[j] = op;
    if (op == 0 || op == 3 || (op >= 4 && op <= 7)) {
      const gpuq_col& c = vals[spec_cols[j]];
      int want = (op == 0 || op == 6 || op == 7) ? GPUQ_FLOAT64 : GPUQ_INT64;
      if (c.dtype != want) FAIL(GPUQ_ERR_INVALID, "aggm: value col dtype mismatch op %d", op);
      cols.p[j] = (const double*)c.data;
      av.v[j] = c.validity;  /* ops skip NULL rows; all-NULL groups stay at
                              * the init acc — callers pair a COUNT spec to
                              * emit SQL NULL (Sum/Min/Max.scala) */
    } else if (op == 1) {
      av.v[j] = vals[spec_cols[j]].validity;
    } else if (op == 8 || op == 10) {
      const gpuq_col& c = vals[spec_cols[j]];
      cols.p[j] = (const double*)c.data;
      av.v[j] = c.validity;  /* op 10: the partial's lo-column validity */
    } else if (op == 9) {
      /* hi column of a 128-bit partial (op 10); unused after op 8 */
      if (spec_ops[j - 1] == 10) cols.p[j] = (const double*)vals[spec_cols[j]].data;
    } else if (op != 2) {
      FAIL(GPUQ_ERR_INVALID, "aggm: bad op %d", op);
    }
  }
  int stride = 1 + nspecs;
  agg_multi_ws w; int64_t need;
  agg_multi_ws_layout(cap, nspecs, &w, (char*)workspace, &need);
  if (first_batch) {
    k_aggm_init<<<grid1d(cap), 256, 0, s>>>(cap, stride, w.tab, ops, w.sp);
    HIP_TRY(hipGetLastError());
  }
  if (n > 0) {
    int64_t lds_bytes = cap * stride * 8;
    bool lds = lds_bytes <= (64 << 10) && getenv("GPUQ_NO_LDS_AGG") == nullptr;
    { hipEvent_t _pe = prof_begin(s);
    if (lds)
      k_aggm_build<true><<<hash_grid(n), 256, (uint32_t)lds_bytes, s>>>(
          n, (const int64_t*)key.data, key.validity, cols, ops, av, nspecs,
          w.tab, w.sp, cap - 1);
    else
      k_aggm_build<false><<<hash_grid(n), 256, 0, s>>>(
          n, (const int64_t*)key.data, key.validity, cols, ops, av, nspecs,
          w.tab, w.sp, cap - 1);
    prof_end("aggm_build", s, _pe); }
    HIP_TRY(hipGetLastError());
  }
  if (finalize) {
    agg_multi_special hsp;
    HIP_TRY(hipMemcpyAsync(&hsp, w.sp, sizeof(hsp), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hsp.overflow) FAIL(GPUQ_ERR_OVERFLOW, "aggm: hash table overflow (capacity %lld)", (long long)cap);
    agg_outs outs = {};
    for (int j = 0; j < nspecs; j++) outs.p[j] = out_accs[j];
    dim3 cgrid((uint32_t)((cap + AGGC_CHUNK - 1) / AGGC_CHUNK));
    k_aggm_compact<<<cgrid, 256, 0, s>>>(cap, w.tab, w.sp, ops, nspecs,
                                         out_keys, out_key_valid, outs);
    HIP_TRY(hipGetLastError());
    agg_multi_special hsp2;
    HIP_TRY(hipMemcpyAsync(&hsp2, w.sp, sizeof(hsp2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out_ngroups = (int64_t)hsp2.out_cursor;
  }
  return GPUQ_OK;
}

/* ============ composite-key hash aggregate (multi-column GROUP BY) ======== */
/*
 * GROUP BY (k1..kK), K <= 4, int64 columns with independent NULLability —
 * the reference groups by an UnsafeRow of the key tuple
 * (UnsafeFixedWidthAggregationMap.java:39, TungstenAggregationIterator.scala:206).
 * Table layout: separate arrays — sig[cap] (u64 claim word), keys[K][cap],
 * kmask[cap] (bit c = key c non-NULL), acc[cap*nspecs]. A slot is claimed by
 * CAS(sig: EMPTY->PENDING), the tuple is published (keys + mask), then the
 * 64-bit signature is released into sig; probers spinning on PENDING retry
 * from the loop head (single attempt per iteration — wave64 lockstep-safe,
 * the publisher's branch always executes between iterations). Tuple equality
 * is verified against the published keys, so signature collisions only cost
 * extra probes, never correctness. No special slots needed: EMPTY/PENDING
 * are reserved signature values no tuple maps to (remapped), so the full
 * int64^K x NULL domain is exact.
 */

#define AGG_MAX_KEYS 4
#define AGGK_EMPTY 0ULL
#define AGGK_PENDING 1ULL

struct agg_keycols { const int64_t* k[AGG_MAX_KEYS]; const uint8_t* v[AGG_MAX_KEYS]; };
struct gpuq_outcols { void* p[AGG_MAX_KEYS]; };

struct aggk_ws {
  unsigned long long* sig;   /* [cap] */
  int64_t* keys;             /* [nkeys][cap] */
  uint8_t* kmask;            /* [cap] */
  unsigned long long* acc;   /* [cap][nspecs] */
  agg_multi_special* sp;     /* out_cursor/overflow only */
};

static void aggk_ws_layout(int64_t cap, int nkeys, int nspecs, aggk_ws* w,
                           char* base, int64_t* total) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->sig = (unsigned long long*)take(cap * 8);
  w->keys = (int64_t*)take(cap * 8 * nkeys);
  w->kmask = (uint8_t*)take(cap);
  w->acc = (unsigned long long*)take(cap * 8 * nspecs);
  w->sp = (agg_multi_special*)take(sizeof(agg_multi_special));
  *total = off;
}

extern "C" int64_t gpuq_hash_agg_keys_workspace_bytes(int64_t cap, int32_t nkeys,
                                                      int32_t nspecs) {
  aggk_ws w; int64_t total;
  aggk_ws_layout(cap, nkeys, nspecs, &w, nullptr, &total);
  return total;
}

__global__ void k_aggk_init(int64_t cap, int nspecs, agg_ops_spec ops,
                            unsigned long long* sig, unsigned long long* acc,
                            agg_multi_special* sp) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < cap; i += gs) {
    sig[i] = AGGK_EMPTY;
    for (int j = 0; j < nspecs; j++)
      acc[(int64_t)nspecs * i + j] = aggm_acc_init(ops.op[j]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sp->out_cursor = 0;
    sp->overflow = 0;
  }
}

/* slot index: the reference's own seed-chained Murmur3 over the key tuple
 * (hash.scala:849-860 HashExpression.eval: NULL leaves the running hash
 * unchanged); signature: splitmix64 chain over (value|NULL-token) pairs. */
DEV void aggk_hash(const agg_keycols kc, int nkeys, int64_t i,
                   uint32_t* slot_hash, unsigned long long* sig, uint8_t* mask) {
  uint32_t h = 42;
  uint64_t s = 0x243F6A8885A308D3ULL;
  uint8_t m = 0;
  for (int c = 0; c < nkeys; c++) {
    bool kv = bit_valid(kc.v[c], i);
    int64_t k = kv ? kc.k[c][i] : 0;
    if (kv) { h = (uint32_t)mm3_hash_long(k, (int32_t)h); m |= (uint8_t)(1 << c); }
    s = splitmix64((s ^ (kv ? (uint64_t)k : 0xD1B54A32D192ED03ULL)) + (uint64_t)c);
  }
  if (s == AGGK_EMPTY || s == AGGK_PENDING) s = 2;
  *slot_hash = h; *sig = s; *mask = m;
}

__global__ __launch_bounds__(256)
void k_aggk_build(int64_t n, agg_keycols kc, int nkeys,
                  agg_cols cols, agg_ops_spec ops, agg_valid av, int nspecs,
                  unsigned long long* sig, int64_t* tkeys, uint8_t* tkmask,
                  unsigned long long* acc, agg_multi_special* sp,
                  int64_t cap, int64_t cap_mask) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) {
    uint32_t h; unsigned long long mysig; uint8_t m;
    aggk_hash(kc, nkeys, i, &h, &mysig, &m);
    uint64_t slot = h & (uint64_t)cap_mask;
    int64_t probes = 0;
    for (;;) {
      unsigned long long cur = __hip_atomic_load(&sig[slot], __ATOMIC_ACQUIRE,
                                                 __HIP_MEMORY_SCOPE_AGENT);
      if (cur == AGGK_EMPTY) {
        unsigned long long prev = atomicCAS(&sig[slot], AGGK_EMPTY, AGGK_PENDING);
        if (prev == AGGK_EMPTY) {
          for (int c = 0; c < nkeys; c++)
            tkeys[(int64_t)c * cap + slot] =
                bit_valid(kc.v[c], i) ? kc.k[c][i] : 0;
          tkmask[slot] = m;
          __hip_atomic_store(&sig[slot], mysig, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        continue;  /* lost the claim: reload (sees PENDING or a sig) */
      }
      if (cur == AGGK_PENDING) continue;  /* publisher runs between iterations */
      if (cur == mysig) {
        bool eq = tkmask[slot] == m;
        for (int c = 0; eq && c < nkeys; c++)
          if ((m >> c) & 1)
            eq = tkeys[(int64_t)c * cap + slot] == kc.k[c][i];
        if (eq) break;
      }
      slot = (slot + 1) & (uint64_t)cap_mask;
      if (++probes > cap_mask) { atomicMax(&sp->overflow, 1ull); return; }
    }
    aggm_update(&acc[(int64_t)nspecs * slot], nspecs, ops, cols, av, i);
  }
}

__global__ void k_aggk_compact(int64_t cap, int nkeys, int nspecs,
                               const unsigned long long* sig, const int64_t* tkeys,
                               const uint8_t* tkmask, const unsigned long long* acc,
                               agg_multi_special* sp, agg_ops_spec ops,
                               gpuq_outcols okeys, uint8_t* out_kmask,
                               agg_outs outs) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & (WAVE - 1);
  for (; i - lane < cap; i += gs) {   /* whole waves iterate together */
    bool occ = i < cap && sig[i] > AGGK_PENDING;
    uint64_t mask = __ballot(occ);
    if (!mask) continue;
    int cnt = __popcll(mask);
    unsigned long long base = 0;
    if (lane == __ffsll((unsigned long long)mask) - 1)
      base = atomicAdd(&sp->out_cursor, (unsigned long long)cnt);
    base = __shfl(base, __ffsll((unsigned long long)mask) - 1);
    if (!occ) continue;
    int64_t o = (int64_t)base + __popcll(mask & ((1ULL << lane) - 1));
    for (int c = 0; c < nkeys; c++)
      ((int64_t*)okeys.p[c])[o] = tkeys[(int64_t)c * cap + i];
    out_kmask[o] = tkmask[i];
    for (int j = 0; j < nspecs; j++)
      aggm_emit(outs.p[j], o, ops.op[j], acc[(int64_t)nspecs * i + j]);
  }
}

extern "C" int gpuq_hash_agg_keys(void* stream, int64_t n,
                                  const gpuq_col* key_cols, int32_t nkeys,
                                  const gpuq_col* vals, const int32_t* spec_ops,
                                  const int32_t* spec_cols, int32_t nspecs,
                                  void* workspace, int64_t cap,
                                  int32_t first_batch, int32_t finalize,
                                  void* const* out_keys, uint8_t* out_kmask,
                                  void* const* out_accs, int64_t* out_ngroups) {
  hipStream_t s = (hipStream_t)stream;
  if (cap <= 0 || (cap & (cap - 1)))
    FAIL(GPUQ_ERR_INVALID, "aggk: capacity %lld not a power of two", (long long)cap);
  if (nkeys < 1 || nkeys > AGG_MAX_KEYS)
    FAIL(GPUQ_ERR_INVALID, "aggk: nkeys %d not in [1,%d]", nkeys, AGG_MAX_KEYS);
  if (nspecs < 1 || nspecs > AGG_MAX_SPECS)
    FAIL(GPUQ_ERR_INVALID, "aggk: nspecs %d not in [1,%d]", nspecs, AGG_MAX_SPECS);
  agg_keycols kc = {};
  for (int c = 0; c < nkeys; c++) {
    if (key_cols[c].dtype != GPUQ_INT64)
      FAIL(GPUQ_ERR_INVALID, "aggk: key col %d must be int64", c);
    kc.k[c] = (const int64_t*)key_cols[c].data;
    kc.v[c] = key_cols[c].validity;
  }
  if (int rc = agg_dec128_check("aggk", vals, spec_ops, spec_cols, nspecs)) return rc;
  agg_cols cols = {}; agg_ops_spec ops = {}; agg_valid av = {};
  for (int j = 0; j < nspecs; j++) {
    int op = spec_ops[j];
    ops.op[j] = op;
    if (op == 0 || op == 3 || (op >= 4 && op <= 7)) {
      const gpuq_col& c = vals[spec_cols[j]];
      int want = (op == 0 || op == 6 || op == 7) ? GPUQ_FLOAT64 : GPUQ_INT64;
      if (c.dtype != want) FAIL(GPUQ_ERR_INVALID, "aggk: value col dtype mismatch op %d", op);
      cols.p[j] = (const double*)c.data;
      av.v[j] = c.validity;
    } else if (op == 1) {
      av.v[j] = vals[spec_cols[j]].validity;
    } else if (op == 8 || op == 10) {
      const gpuq_col& c = vals[spec_cols[j]];
      cols.p[j] = (const double*)c.data;
      av.v[j] = c.validity;  /* op 10: the partial's lo-column validity */
    } else if (op == 9) {
      /* hi column of a 128-bit partial (op 10); unused after op 8 */
      if (spec_ops[j - 1] == 10) cols.p[j] = (const double*)vals[spec_cols[j]].data;
    } else if (op != 2) {
      FAIL(GPUQ_ERR_INVALID, "aggk: bad op %d", op);
    }
  }
  aggk_ws w; int64_t need;
  aggk_ws_layout(cap, nkeys, nspecs, &w, (char*)workspace, &need);
  if (first_batch) {
    k_aggk_init<<<grid1d(cap), 256, 0, s>>>(cap, nspecs, ops, w.sig, w.acc, w.sp);
    HIP_TRY(hipGetLastError());
  }
  if (n > 0) {
    { hipEvent_t _pe = prof_begin(s);
    k_aggk_build<<<hash_grid(n), 256, 0, s>>>(
        n, kc, nkeys, cols, ops, av, nspecs, w.sig, w.keys, w.kmask, w.acc,
        w.sp, cap, cap - 1);
    prof_end("aggk_build", s, _pe); }
    HIP_TRY(hipGetLastError());
  }
  if (finalize) {
    agg_multi_special hsp;
    HIP_TRY(hipMemcpyAsync(&hsp, w.sp, sizeof(hsp), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hsp.overflow) FAIL(GPUQ_ERR_OVERFLOW, "aggk: hash table overflow (capacity %lld)", (long long)cap);
    gpuq_outcols okeys = {};
    for (int c = 0; c < nkeys; c++) okeys.p[c] = (void*)out_keys[c];
    agg_outs outs = {};
    for (int j = 0; j < nspecs; j++) outs.p[j] = (void*)out_accs[j];
    k_aggk_compact<<<grid1d(cap), 256, 0, s>>>(cap, nkeys, nspecs, w.sig, w.keys,
                                               w.kmask, w.acc, w.sp, ops, okeys,
                                               out_kmask, outs);
    HIP_TRY(hipGetLastError());
    agg_multi_special hsp2;
    HIP_TRY(hipMemcpyAsync(&hsp2, w.sp, sizeof(hsp2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out_ngroups = (int64_t)hsp2.out_cursor;
  }
  return GPUQ_OK;
}

/* ============ multi-column partition ids (seed-chained Murmur3) =========== */
/* pid = Pmod(Murmur3Hash(k1..kK, 42), n) with the hash chained column-wise
 * and NULL columns passing the running seed through unchanged —
 * HashPartitioning.partitionIdExpression (partitioning.scala:328) over
 * HashExpression.eval (hash.scala:849-860). */

__global__ void k_partition_pids_multi(int64_t n, agg_keycols kc, int nkeys,
                                       int32_t nparts, uint64_t* pid_as_key,
                                       uint32_t* idx,
                                       unsigned long long* counts) {
  __shared__ uint32_t h[256];
  bool lds_counts = nparts <= 256;
  if (lds_counts)
    for (int b = threadIdx.x; b < nparts; b += blockDim.x) h[b] = 0;
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int32_t hsh = 42;
    for (int c = 0; c < nkeys; c++)
      if (bit_valid(kc.v[c], i)) hsh = mm3_hash_long(kc.k[c][i], hsh);
    int pid = spark_pmod(hsh, nparts);
    pid_as_key[i] = (uint64_t)pid;
    idx[i] = (uint32_t)i;
    if (lds_counts) atomicAdd(&h[pid], 1u);
    else atomicAdd(&counts[pid], 1ull);
  }
  __syncthreads();
  if (lds_counts)
    for (int b = threadIdx.x; b < nparts; b += blockDim.x)
      if (h[b]) atomicAdd(&counts[b], (unsigned long long)h[b]);
}

/* shared tail of the partition entry points: stable radix over the pid */
static int partition_scatter_tail(hipStream_t s, int64_t n, sort_ws& w,
                                  int32_t nparts, uint32_t* out_perm) {
  scatter_geom geom = get_sort_geom();
  int tile = geom.block * geom.items;
  int64_t nb = sort_nblocks(n, tile);
  int passes = nparts > 256 ? 2 : 1;
  uint64_t *kin = w.ka, *kout = w.kb;
  uint32_t *iin = w.ia, *iout = w.ib;
  for (int p = 0; p < passes; p++) {
    { hipEvent_t _pe = prof_begin(s);
    k_radix_hist<0><<<dim3((uint32_t)nb), 256, 0, s>>>(n, kin, p * 8, w.hist, (int)nb, tile);
    prof_end("radix_hist", s, _pe); }
    HIP_TRY(hipGetLastError());
    int rc = exclusive_scan_u32(s, (int64_t)256 * nb, w.hist, w.hist_scan, w.block_sums);
    if (rc) return rc;
    uint32_t* iout_pass = (p == passes - 1) ? out_perm : iout;
    { hipEvent_t _pe = prof_begin(s);
    launch_scatter<0, false>(s, geom, nb, n, kin, iin, kout, iout_pass, w.hist_scan,
                             p * 8, 0, nullptr, nullptr, nullptr, 0);
    prof_end("radix_scatter", s, _pe); }
    HIP_TRY(hipGetLastError());
    uint64_t* tk = kin; kin = kout; kout = tk;
    uint32_t* ti = iin; iin = iout_pass; iout = ti;
  }
  return GPUQ_OK;
}

extern "C" int gpuq_partition_perm_multi(void* stream, int64_t n,
                                         const gpuq_col* key_cols, int32_t nkeys,
                                         int32_t nparts, uint32_t* out_perm,
                                         int64_t* out_counts,
                                         void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n > 0xFFFFFFFFLL) FAIL(GPUQ_ERR_INVALID, "partition: nrows %lld > 2^32", (long long)n);
  if (nparts < 1 || nparts > 65536)
    FAIL(GPUQ_ERR_INVALID, "partition: num_parts %d not in [1,65536]", nparts);
  if (nkeys < 1 || nkeys > AGG_MAX_KEYS)
    FAIL(GPUQ_ERR_INVALID, "partition: nkeys %d not in [1,%d]", nkeys, AGG_MAX_KEYS);
  agg_keycols kc = {};
  for (int c = 0; c < nkeys; c++) {
    if (key_cols[c].dtype != GPUQ_INT64)
      FAIL(GPUQ_ERR_INVALID, "partition: key col %d must be int64", c);
    kc.k[c] = (const int64_t*)key_cols[c].data;
    kc.v[c] = key_cols[c].validity;
  }
  sort_ws w; int64_t need;
  sort_ws_layout(n, 256, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "partition: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
  HIP_TRY(hipMemsetAsync(out_counts, 0, (size_t)nparts * 8, s));
  if (n == 0) return GPUQ_OK;
  { hipEvent_t _pe = prof_begin(s);
  k_partition_pids_multi<<<grid1d(n), 256, 0, s>>>(n, kc, nkeys, nparts, w.ka, w.ia,
                                                   (unsigned long long*)out_counts);
  prof_end("partition_pids", s, _pe); }
  HIP_TRY(hipGetLastError());
  return partition_scatter_tail(s, n, w, nparts, out_perm);
}

/* out[i] = col[perm[i]] with perm[i] == 0xFFFFFFFF (JOIN_NIL) producing a
 * NULL output row (outer-join build side); out_bits = resulting validity
 * (src validity AND not-NIL). */
__global__ void k_gather_nullable(int64_t n, const uint64_t* col,
                                  const uint8_t* src_valid,
                                  const uint32_t* perm, uint64_t* out,
                                  uint8_t* out_bits) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nbytes = (n + 7) >> 3;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; b < nbytes; b += gs) {
    uint8_t v = 0;
    int64_t row0 = b << 3;
    int top = (int)((n - row0) < 8 ? (n - row0) : 8);
    for (int t = 0; t < top; t++) {
      uint32_t p = perm[row0 + t];
      bool ok = p != 0xFFFFFFFFu;
      out[row0 + t] = ok ? col[p] : 0;
      if (ok && (!src_valid || ((src_valid[p >> 3] >> (p & 7)) & 1)))
        v |= (uint8_t)(1 << t);
    }
    out_bits[b] = v;
  }
}

extern "C" int gpuq_gather_nullable(void* stream, int64_t nrows, gpuq_col col,
                                    const uint32_t* perm, void* out,
                                    uint8_t* out_bits) {
  hipStream_t s = (hipStream_t)stream;
  if (col.dtype != GPUQ_INT64 && col.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "gather_nullable: unsupported dtype %d", col.dtype);
  if (nrows == 0) return GPUQ_OK;
  int64_t nbytes = (nrows + 7) >> 3;
  k_gather_nullable<<<grid1d(nbytes), 256, 0, s>>>(
      nrows, (const uint64_t*)col.data, col.validity, perm, (uint64_t*)out,
      out_bits);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ================= validity-bitmap utilities ================= */
/* The ColumnVector contract carries NULLs everywhere (ColumnVector.java:
 * 58-366); these kernels move Arrow validity bitmaps (LSB-first) through
 * permutations and across the exchange (bitmaps travel as u8 columns in
 * the all-to-all because row split points are not byte-aligned). */

__global__ void k_gather_bits(int64_t n, const uint8_t* src, const uint32_t* perm,
                              uint8_t* out) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   /* output byte */
  int64_t nbytes = (n + 7) >> 3;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; b < nbytes; b += gs) {
    uint8_t v = 0;
    int64_t row0 = b << 3;
    int top = (int)((n - row0) < 8 ? (n - row0) : 8);
    for (int t = 0; t < top; t++) {
      uint32_t p = perm[row0 + t];
      v |= (uint8_t)(((src[p >> 3] >> (p & 7)) & 1) << t);
    }
    out[b] = v;
  }
}

extern "C" int gpuq_gather_bits(void* stream, int64_t nrows, const uint8_t* src_bits,
                                const uint32_t* perm, uint8_t* out_bits) {
  hipStream_t s = (hipStream_t)stream;
  if (nrows == 0) return GPUQ_OK;
  int64_t nbytes = (nrows + 7) >> 3;
  k_gather_bits<<<grid1d(nbytes), 256, 0, s>>>(nrows, src_bits, perm, out_bits);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

__global__ void k_bits_to_u8(int64_t n, const uint8_t* bits, uint8_t* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) out[i] = (bits[i >> 3] >> (i & 7)) & 1;
}

extern "C" int gpuq_bits_to_u8(void* stream, int64_t nrows, const uint8_t* bits,
                               uint8_t* out) {
  hipStream_t s = (hipStream_t)stream;
  if (nrows == 0) return GPUQ_OK;
  k_bits_to_u8<<<grid1d(nrows), 256, 0, s>>>(nrows, bits, out);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

__global__ void k_u8_to_bits(int64_t n, const uint8_t* u8, uint8_t* bits) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nbytes = (n + 7) >> 3;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; b < nbytes; b += gs) {
    uint8_t v = 0;
    int64_t row0 = b << 3;
    int top = (int)((n - row0) < 8 ? (n - row0) : 8);
    for (int t = 0; t < top; t++) v |= (uint8_t)((u8[row0 + t] & 1) << t);
    bits[b] = v;
  }
}

extern "C" int gpuq_u8_to_bits(void* stream, int64_t nrows, const uint8_t* u8,
                               uint8_t* out_bits) {
  hipStream_t s = (hipStream_t)stream;
  if (nrows == 0) return GPUQ_OK;
  int64_t nbytes = (nrows + 7) >> 3;
  k_u8_to_bits<<<grid1d(nbytes), 256, 0, s>>>(nrows, u8, out_bits);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

__global__ void k_nonzero_to_bits(int64_t n, const int64_t* in, uint8_t* bits) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nbytes = (n + 7) >> 3;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; b < nbytes; b += gs) {
    uint8_t v = 0;
    int64_t row0 = b << 3;
    int top = (int)((n - row0) < 8 ? (n - row0) : 8);
    for (int t = 0; t < top; t++) v |= (uint8_t)((in[row0 + t] != 0 ? 1 : 0) << t);
    bits[b] = v;
  }
}

/* validity bitmap from an int64 column: bit i = (in[i] != 0). Used to turn
 * merged partial COUNTs into the NULL-ness of merged SUM/MIN/MAX results
 * (Sum.scala: result is NULL iff no non-null input). */
extern "C" int gpuq_nonzero_to_bits(void* stream, int64_t nrows, const int64_t* in,
                                    uint8_t* out_bits) {
  hipStream_t s = (hipStream_t)stream;
  if (nrows == 0) return GPUQ_OK;
  int64_t nbytes = (nrows + 7) >> 3;
  k_nonzero_to_bits<<<grid1d(nbytes), 256, 0, s>>>(nrows, in, out_bits);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* one thread owns one validity byte (8 rows): no two threads write a byte */
__global__ void k_dec128_overflow_to_null(int64_t n, const int64_t* lo,
                                          const int64_t* hi,
                                          unsigned long long blo,
                                          unsigned long long bhi, uint8_t* bits) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nbytes = (n + 7) >> 3;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; b < nbytes; b += gs) {
    uint8_t keep = 0;
    int64_t row0 = b << 3;
    int top = (int)((n - row0) < 8 ? (n - row0) : 8);
    for (int t = 0; t < top; t++) {
      unsigned long long l = (unsigned long long)lo[row0 + t];
      unsigned long long h = (unsigned long long)hi[row0 + t];
      if ((long long)h < 0) {  /* |x| as u128 (2^127 stays 2^127) */
        h = ~h + (l == 0);
        l = ~l + 1;
      }
      bool fits = h < bhi || (h == bhi && l < blo);
      keep |= (uint8_t)((fits ? 1 : 0) << t);
    }
    bits[b] &= (uint8_t)(keep | (0xFF << top));
  }
}

/* Sum.scala non-ANSI decimal overflow: the 128-bit sum (hi,lo) becomes NULL
 * when it no longer fits decimal(result_precision, s), i.e. clears validity
 * bit i unless -10^p < x < 10^p. Bits already clear stay clear. */
extern "C" int gpuq_dec128_overflow_to_null(void* stream, int64_t nrows,
                                            const int64_t* lo, const int64_t* hi,
                                            int32_t result_precision,
                                            uint8_t* validity_bits) {
  hipStream_t s = (hipStream_t)stream;
  if (result_precision < 1 || result_precision > 38)
    FAIL(GPUQ_ERR_INVALID, "dec128: result precision %d not in [1,38]", result_precision);
  if (nrows == 0) return GPUQ_OK;
  unsigned __int128 bound = 1;
  for (int d = 0; d < result_precision; d++) bound *= 10;
  int64_t nbytes = (nrows + 7) >> 3;
  k_dec128_overflow_to_null<<<grid1d(nbytes), 256, 0, s>>>(
      nrows, lo, hi, (unsigned long long)bound, (unsigned long long)(bound >> 64),
      validity_bits);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

__global__ void k_maskbit_to_bits(int64_t n, const uint8_t* mask, int bit,
                                  uint8_t* bits) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nbytes = (n + 7) >> 3;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; b < nbytes; b += gs) {
    uint8_t v = 0;
    int64_t row0 = b << 3;
    int top = (int)((n - row0) < 8 ? (n - row0) : 8);
    for (int t = 0; t < top; t++)
      v |= (uint8_t)(((mask[row0 + t] >> bit) & 1) << t);
    bits[b] = v;
  }
}

/* validity bitmap for key column `bit` from gpuq_hash_agg_keys' out_kmask */
extern "C" int gpuq_maskbit_to_bits(void* stream, int64_t nrows,
                                    const uint8_t* mask, int32_t bit,
                                    uint8_t* out_bits) {
  hipStream_t s = (hipStream_t)stream;
  if (bit < 0 || bit > 7) FAIL(GPUQ_ERR_INVALID, "maskbit: bit %d", bit);
  if (nrows == 0) return GPUQ_OK;
  int64_t nbytes = (nrows + 7) >> 3;
  k_maskbit_to_bits<<<grid1d(nbytes), 256, 0, s>>>(nrows, mask, bit, out_bits);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ================= min/max reduction (int64 column) ================= */
/* out_dev[0] = min (encoded u64), out_dev[1] = max (encoded), out_dev[2] =
 * count of valid rows. Used by the host packing rule (narrow composite keys
 * -> one i64) and for range sanity checks. */

__global__ void k_minmax_i64(int64_t n, const int64_t* data, const uint8_t* validity,
                             unsigned long long* out) {
  __shared__ unsigned long long smin[256], smax[256];
  __shared__ unsigned long long scnt;
  if (threadIdx.x == 0) scnt = 0;
  unsigned long long lmin = ~0ULL, lmax = 0, lcnt = 0;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) {
    if (!bit_valid(validity, i)) continue;
    unsigned long long e = encode_i64(data[i]);
    if (e < lmin) lmin = e;
    if (e > lmax) lmax = e;
    lcnt++;
  }
  smin[threadIdx.x] = lmin; smax[threadIdx.x] = lmax;
  __syncthreads();
  if (lcnt) atomicAdd(&scnt, lcnt);
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      if (smin[threadIdx.x + w] < smin[threadIdx.x]) smin[threadIdx.x] = smin[threadIdx.x + w];
      if (smax[threadIdx.x + w] > smax[threadIdx.x]) smax[threadIdx.x] = smax[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicMin(&out[0], smin[0]);
    atomicMax(&out[1], smax[0]);
    if (scnt) atomicAdd(&out[2], scnt);
  }
}

extern "C" int gpuq_minmax_i64(void* stream, int64_t nrows, gpuq_col col,
                               unsigned long long* out_dev /* [3] */) {
  hipStream_t s = (hipStream_t)stream;
  if (col.dtype != GPUQ_INT64) FAIL(GPUQ_ERR_INVALID, "minmax: col must be int64");
  HIP_TRY(hipMemsetAsync(out_dev, 0xFF, 8, s));       /* min := u64 max */
  HIP_TRY(hipMemsetAsync(out_dev + 1, 0, 16, s));     /* max := 0, cnt := 0 */
  if (nrows == 0) return GPUQ_OK;
  k_minmax_i64<<<grid1d(nrows), 256, 0, s>>>(nrows, (const int64_t*)col.data,
                                             col.validity, out_dev);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ================= narrow-key pack/unpack ================= */
/* Pack two int64 key columns with known small ranges into one int64:
 * out = (a - a_bias) << shift | (b - b_bias). The host rule verifies
 * 0 <= a-a_bias < 2^(63-shift) and 0 <= b-b_bias < 2^shift via
 * gpuq_minmax_i64 first; the packed key feeds the fast single-key
 * aggregation path (LDS tables at low cardinality), then unpack restores
 * the tuple. NULLs must be handled by the caller (packing is only applied
 * to non-null key columns). */

__global__ void k_pack2_i64(int64_t n, const int64_t* a, const int64_t* b,
                            int64_t a_bias, int64_t b_bias, int shift,
                            int64_t* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs)
    out[i] = ((a[i] - a_bias) << shift) | (b[i] - b_bias);
}

extern "C" int gpuq_pack2_i64(void* stream, int64_t nrows, const int64_t* a,
                              const int64_t* b, int64_t a_bias, int64_t b_bias,
                              int32_t shift, int64_t* out) {
  hipStream_t s = (hipStream_t)stream;
  if (shift < 1 || shift > 62) FAIL(GPUQ_ERR_INVALID, "pack2: shift %d", shift);
  if (nrows == 0) return GPUQ_OK;
  k_pack2_i64<<<grid1d(nrows), 256, 0, s>>>(nrows, a, b, a_bias, b_bias, shift, out);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

__global__ void k_unpack2_i64(int64_t n, const int64_t* in, int64_t a_bias,
                              int64_t b_bias, int shift, int64_t* a, int64_t* b) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += gs) {
    int64_t v = in[i];
    if (a) a[i] = (v >> shift) + a_bias;
    if (b) b[i] = (v & (((int64_t)1 << shift) - 1)) + b_bias;
  }
}

extern "C" int gpuq_unpack2_i64(void* stream, int64_t nrows, const int64_t* in,
                                int64_t a_bias, int64_t b_bias, int32_t shift,
                                int64_t* out_a, int64_t* out_b) {
  hipStream_t s = (hipStream_t)stream;
  if (shift < 1 || shift > 62) FAIL(GPUQ_ERR_INVALID, "unpack2: shift %d", shift);
  if (nrows == 0) return GPUQ_OK;
  k_unpack2_i64<<<grid1d(nrows), 256, 0, s>>>(nrows, in, a_bias, b_bias, shift,
                                              out_a, out_b);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ================= filter / project (SURVEY (f).2) ================= */
/*
 * FILTER — replaces FilterExec for single-comparison predicates
 * (col OP literal): stable compaction via the same ranked-scatter machinery
 * as the sort's validity split (pass=group 0, fail=group 1; WHERE keeps
 * only TRUE — a NULL comparison result drops the row, SQL 3VL).
 * PROJECT — replaces ProjectExec for elementwise binary arithmetic
 * (col OP col / col OP literal) on int64/float64.
 */

/* float64 follows Spark's total order (SQLOrderingUtil.compareDoubles), the
 * same one the sort and MIN/MAX use: NaN == NaN and NaN is greater than every
 * other value, +inf included; -0.0 == 0.0. Non-NaN operands take the plain
 * IEEE comparison below. */
DEV bool filter_cmp_f64(double v, int op, double lit) {
  if (v != v || lit != lit) {
    bool vn = v != v, ln = lit != lit;
    int c = (vn && ln) ? 0 : (vn ? 1 : -1);
    switch (op) {
      case 0: return c == 0;
      case 1: return c < 0;
      case 2: return c <= 0;
      case 3: return c > 0;
      case 4: return c >= 0;
      default: return c != 0;
    }
  }
  switch (op) {
    case 0: return v == lit;
    case 1: return v < lit;
    case 2: return v <= lit;
    case 3: return v > lit;
    case 4: return v >= lit;
    default: return v != lit;
  }
}
DEV bool filter_cmp_i64(int64_t v, int op, int64_t lit) {
  switch (op) {
    case 0: return v == lit;
    case 1: return v < lit;
    case 2: return v <= lit;
    case 3: return v > lit;
    case 4: return v >= lit;
    default: return v != lit;
  }
}

template <int DTYPE>
__global__ void k_filter_pred(int64_t n, const void* data, const uint8_t* validity,
                              int op, double lit_f, int64_t lit_i,
                              uint64_t* pid_as_key, uint32_t* idx,
                              unsigned long long* pass_count) {
  __shared__ unsigned int h;
  if (threadIdx.x == 0) h = 0;
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int mine = 0;
  for (; i < n; i += stride) {
    bool pass = bit_valid(validity, i);
    if (pass) {
      if (DTYPE == GPUQ_FLOAT64) pass = filter_cmp_f64(((const double*)data)[i], op, lit_f);
      else pass = filter_cmp_i64(((const int64_t*)data)[i], op, lit_i);
    }
    pid_as_key[i] = pass ? 0ull : 1ull;
    idx[i] = (uint32_t)i;
    if (pass) mine++;
  }
  if (mine) atomicAdd(&h, mine);
  __syncthreads();
  if (threadIdx.x == 0 && h) atomicAdd(pass_count, (unsigned long long)h);
}

extern "C" int64_t gpuq_filter_workspace_bytes(int64_t n) {
  return gpuq_sort_workspace_bytes(n);
}

extern "C" int gpuq_filter_cmp(void* stream, int64_t n, gpuq_col col, int32_t op,
                               double lit_f, int64_t lit_i,
                               uint32_t* out_perm, int64_t* out_count,
                               void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n > 0xFFFFFFFFLL) FAIL(GPUQ_ERR_INVALID, "filter: nrows %lld > 2^32", (long long)n);
  if (op < 0 || op > 5) FAIL(GPUQ_ERR_INVALID, "filter: bad op %d", op);
  if (col.dtype != GPUQ_INT64 && col.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "filter: unsupported dtype %d", col.dtype);
  sort_ws w; int64_t need;
  sort_ws_layout(n, 256, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "filter: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
  HIP_TRY(hipMemsetAsync(out_count, 0, 8, s));
  if (n == 0) return GPUQ_OK;
  scatter_geom geom = get_sort_geom();
  int tile = geom.block * geom.items;
  int64_t nb = sort_nblocks(n, tile);
  { hipEvent_t _pe = prof_begin(s);
  if (col.dtype == GPUQ_FLOAT64)
    k_filter_pred<GPUQ_FLOAT64><<<grid1d(n), 256, 0, s>>>(
        n, col.data, col.validity, op, lit_f, lit_i, w.ka, w.ia,
        (unsigned long long*)out_count);
  else
    k_filter_pred<GPUQ_INT64><<<grid1d(n), 256, 0, s>>>(
        n, col.data, col.validity, op, lit_f, lit_i, w.ka, w.ia,
        (unsigned long long*)out_count);
  prof_end("filter_pred", s, _pe); }
  HIP_TRY(hipGetLastError());
  k_radix_hist<0><<<dim3((uint32_t)nb), 256, 0, s>>>(n, w.ka, 0, w.hist, (int)nb, tile);
  HIP_TRY(hipGetLastError());
  int rc = exclusive_scan_u32(s, 256 * nb, w.hist, w.hist_scan, w.block_sums);
  if (rc) return rc;
  { hipEvent_t _pe = prof_begin(s);
  launch_scatter<0, false>(s, geom, nb, n, w.ka, w.ia, w.kb, w.ib, w.hist_scan,
                           0, 0, nullptr, nullptr, nullptr, 0);
  prof_end("filter_scatter", s, _pe); }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_perm, w.ib, n * 4, hipMemcpyDeviceToDevice, s));
  return GPUQ_OK;
}

/* ---- compound predicates: one fused pass (gpuq_filter_expr) ----
 *
 *  mask  k_pred_mask: one block per PRED_TILE rows interprets the postfix
 *        program over its rows and writes one pass bit per row (a 64-bit
 *        ballot word per wave and round) plus the block's pass count.
 *  scan  exclusive_scan_u32 over the block counts.
 *  emit  k_pred_emit: reads only its tile's mask words and writes the row id
 *        of every set bit at scan[block] + rank inside the tile.
 * Two bounded phases, no lookback and no spin (the top-k emit's shape). The
 * columns are read once, by the mask kernel.
 */
#define PRED_BLOCK 256
#define PRED_WAVES (PRED_BLOCK / WAVE)
#define PRED_ITEMS 8
#define PRED_TILE (PRED_BLOCK * PRED_ITEMS)   /* 2048 rows per block */
#define PRED_WORDS (PRED_TILE / WAVE)         /* 32 mask words per block */

/* column table and program, passed by value in the kernel arguments */
struct pred_args {
  const void* data[GPUQ_PRED_MAX_COLS];
  const uint8_t* validity[GPUQ_PRED_MAX_COLS];
  int32_t dtype[GPUQ_PRED_MAX_COLS];
  int32_t ninsns;
  gpuq_pred_insn insn[GPUQ_PRED_MAX_INSNS];
};

static void pred_fill_args(pred_args* a, const gpuq_col* cols, int32_t ncols,
                           const gpuq_pred_insn* prog, int32_t ninsns) {
  memset(a, 0, sizeof(*a));
  for (int c = 0; c < ncols; c++) {
    a->data[c] = cols[c].data;
    a->validity[c] = cols[c].validity;
    a->dtype[c] = cols[c].dtype;
  }
  for (int pc = 0; pc < ninsns; pc++) a->insn[pc] = prog[pc];
  a->ninsns = ninsns;
}

/* The interpreter: runs a validated program (pred_check_program: it never
 * pops an empty stack) for R rows per thread and leaves row r's result in
 * bit 0 of tb[r]. load(c, v) fetches column c for the thread's R rows: the
 * values into v[], the validity bits (bit r = row r) as its result.
 *
 * The program counter is the same in every lane (the program comes from the
 * kernel arguments), so the interpreter's branches are wave-uniform.
 * Instructions outer, the R rows inner and unrolled: a leaf issues its R
 * loads back to back.
 *
 * The per-row evaluation stack is two 32-bit words: bit d of tb[r] / nb[r] is
 * the TRUE / NULL flag of stack slot d (slot 0 = top; never both set; both
 * clear = FALSE). A push shifts left and ors the new flag in; AND / OR / NOT
 * rewrite the low bits. Nothing is indexed by a runtime value.
 *
 * cv / cvalid cache the most recently loaded col_a: consecutive leaves on one
 * column — BETWEEN, IN — load it once. */
template <int R, class Load>
DEV void pred_eval(const pred_args& a, Load load, uint32_t (&tb)[R]) {
  uint32_t nb[R];
  uint64_t cv[R];
  uint32_t cvalid = 0;
  int cached = -1;
  #pragma unroll
  for (int r = 0; r < R; r++) { tb[r] = 0; nb[r] = 0; cv[r] = 0; }

  for (int pc = 0; pc < a.ninsns; pc++) {
    const int opcode = a.insn[pc].opcode;
    if (opcode <= GPUQ_PRED_IS_NOT_NULL) {
      const int ca = a.insn[pc].col_a;
      if (ca != cached) {
        cvalid = load(ca, cv);
        cached = ca;
      }
      if (opcode == GPUQ_PRED_CMP_LIT) {
        const int op = a.insn[pc].cmp;
        if (a.dtype[ca] == GPUQ_FLOAT64) {
          const double lit = a.insn[pc].lit_f64;
          #pragma unroll
          for (int r = 0; r < R; r++) {
            uint32_t ok = (cvalid >> r) & 1;
            uint32_t t = filter_cmp_f64(__longlong_as_double((long long)cv[r]), op, lit);
            tb[r] = (tb[r] << 1) | (t & ok);
            nb[r] = (nb[r] << 1) | (ok ^ 1);
          }
        } else {
          const int64_t lit = a.insn[pc].lit_i64;
          #pragma unroll
          for (int r = 0; r < R; r++) {
            uint32_t ok = (cvalid >> r) & 1;
            uint32_t t = filter_cmp_i64((int64_t)cv[r], op, lit);
            tb[r] = (tb[r] << 1) | (t & ok);
            nb[r] = (nb[r] << 1) | (ok ^ 1);
          }
        }
      } else if (opcode == GPUQ_PRED_CMP_COL) {
        const int op = a.insn[pc].cmp;
        const bool f64 = a.dtype[ca] == GPUQ_FLOAT64;
        uint64_t bv[R];
        const uint32_t bvalid = load(a.insn[pc].col_b, bv) & cvalid;
        #pragma unroll
        for (int r = 0; r < R; r++) {
          uint32_t ok = (bvalid >> r) & 1;
          uint32_t t = f64
              ? filter_cmp_f64(__longlong_as_double((long long)cv[r]), op,
                               __longlong_as_double((long long)bv[r]))
              : filter_cmp_i64((int64_t)cv[r], op, (int64_t)bv[r]);
          tb[r] = (tb[r] << 1) | (t & ok);
          nb[r] = (nb[r] << 1) | (ok ^ 1);
        }
      } else {   /* IS_NULL / IS_NOT_NULL */
        const uint32_t flip = opcode == GPUQ_PRED_IS_NULL ? 1u : 0u;
        #pragma unroll
        for (int r = 0; r < R; r++) {
          tb[r] = (tb[r] << 1) | (((cvalid >> r) & 1) ^ flip);
          nb[r] = nb[r] << 1;
        }
      }
    } else if (opcode == GPUQ_PRED_CONST) {
      const uint32_t t = a.insn[pc].cmp == GPUQ_PRED_TRUE;
      const uint32_t nl = a.insn[pc].cmp == GPUQ_PRED_NULL;
      #pragma unroll
      for (int r = 0; r < R; r++) {
        tb[r] = (tb[r] << 1) | t;
        nb[r] = (nb[r] << 1) | nl;
      }
    } else if (opcode == GPUQ_PRED_AND) {
      #pragma unroll
      for (int r = 0; r < R; r++) {
        uint32_t T = tb[r], N = nb[r];
        uint32_t rt = (T >> 1) & T & 1;
        /* NULL unless a side is FALSE: both sides TRUE-or-NULL, one NULL */
        uint32_t rn = ((N >> 1) | N) & ((T >> 1) | (N >> 1)) & (T | N) & 1;
        tb[r] = ((T >> 1) & ~1u) | rt;
        nb[r] = ((N >> 1) & ~1u) | rn;
      }
    } else if (opcode == GPUQ_PRED_OR) {
      #pragma unroll
      for (int r = 0; r < R; r++) {
        uint32_t T = tb[r], N = nb[r];
        uint32_t rt = ((T >> 1) | T) & 1;
        uint32_t rn = ((N >> 1) | N) & ~rt & 1;
        tb[r] = ((T >> 1) & ~1u) | rt;
        nb[r] = ((N >> 1) & ~1u) | rn;
      }
    } else {   /* NOT: FALSE <-> TRUE, NULL stays */
      #pragma unroll
      for (int r = 0; r < R; r++)
        tb[r] = (tb[r] & ~1u) | (~(tb[r] | nb[r]) & 1);
    }
  }
}

/* Row r of thread t is base + r * PRED_BLOCK + t: for each r a wave covers 64
 * consecutive rows, so its ballot is mask word r * PRED_WAVES + wave of the
 * tile and the words ascend in row order. */
__global__ __launch_bounds__(PRED_BLOCK)
void k_pred_mask(int64_t n, pred_args a, unsigned long long* mask, uint32_t* cnt) {
  __shared__ uint32_t wcnt[PRED_WAVES];
  const int64_t base = (int64_t)blockIdx.x * PRED_TILE + threadIdx.x;
  uint32_t tb[PRED_ITEMS];
  pred_eval<PRED_ITEMS>(a, [&](int c, uint64_t (&v)[PRED_ITEMS]) {
    const uint64_t* d = (const uint64_t*)a.data[c];
    const uint8_t* val = a.validity[c];
    uint32_t valid = 0;
    #pragma unroll
    for (int r = 0; r < PRED_ITEMS; r++) {
      int64_t i = base + r * PRED_BLOCK;
      bool in = i < n;
      v[r] = in ? d[i] : 0;
      valid |= (uint32_t)(in && bit_valid(val, i)) << r;
    }
    return valid;
  }, tb);


  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  uint32_t total = 0;
  #pragma unroll
  for (int r = 0; r < PRED_ITEMS; r++) {
    bool pass = (tb[r] & 1) && base + r * PRED_BLOCK < n;
    unsigned long long m = __ballot(pass);
    total += (uint32_t)__popcll(m);
    if (lane == 0)
      mask[(int64_t)blockIdx.x * PRED_WORDS + r * PRED_WAVES + wave] = m;
  }
  if (lane == 0) wcnt[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
    #pragma unroll
    for (int w = 0; w < PRED_WAVES; w++) c += wcnt[w];
    cnt[blockIdx.x] = c;
  }
}

/* scan[b] passing rows precede block b's tile. The block loads its 32 mask
 * words, prefixes their popcounts in LDS (one wave scan), and the lane of
 * each set bit writes its row id at scan[b] + word prefix + rank in the word.
 * At most n bits are set in all (rows >= n contribute 0), so every slot is
 * below n. The last block also writes the total. */
__global__ __launch_bounds__(PRED_BLOCK)
void k_pred_emit(const unsigned long long* mask, const uint32_t* scan,
                 uint32_t nblocks, uint32_t* out_perm,
                 unsigned long long* out_count) {
  __shared__ unsigned long long words[PRED_WORDS];
  __shared__ uint32_t wpre[PRED_WORDS + 1];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  if (wave == 0) {
    unsigned long long m = lane < PRED_WORDS
        ? mask[(int64_t)blockIdx.x * PRED_WORDS + lane] : 0ull;
    uint32_t c = (uint32_t)__popcll(m);
    uint32_t inc = wave_inclusive_scan(c);
    if (lane < PRED_WORDS) { words[lane] = m; wpre[lane] = inc - c; }
    if (lane == PRED_WORDS - 1) wpre[PRED_WORDS] = inc;
  }
  __syncthreads();
  const uint32_t start = scan[blockIdx.x];
  const unsigned long long lt = (1ULL << lane) - 1;
  const int64_t base = (int64_t)blockIdx.x * PRED_TILE + threadIdx.x;
  #pragma unroll
  for (int r = 0; r < PRED_ITEMS; r++) {
    const int w = r * PRED_WAVES + wave;
    unsigned long long m = words[w];
    if ((m >> lane) & 1)
      out_perm[start + wpre[w] + (uint32_t)__popcll(m & lt)] =
          (uint32_t)(base + r * PRED_BLOCK);
  }
  if (blockIdx.x == nblocks - 1 && threadIdx.x == 0)
    *out_count = (unsigned long long)start + wpre[PRED_WORDS];
}

struct pred_ws {
  unsigned long long* mask;  /* [blocks][PRED_WORDS] pass bits */
  uint32_t* cnt;             /* [blocks] pass counts */
  uint32_t* scan;            /* exclusive prefix sums of cnt */
  uint32_t* block_sums;
};

static void pred_ws_layout(int64_t n, pred_ws* w, char* basep, int64_t* total) {
  int64_t nb = (n + PRED_TILE - 1) / PRED_TILE;
  int64_t scan_blocks = (nb + SCAN_TILE - 1) / SCAN_TILE + 1;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = basep ? basep + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->mask = (unsigned long long*)take(nb * PRED_WORDS * 8);
  w->cnt = (uint32_t*)take(nb * 4);
  w->scan = (uint32_t*)take(nb * 4);
  w->block_sums = (uint32_t*)take(scan_blocks * 4);
  *total = off;
}

extern "C" int64_t gpuq_filter_expr_workspace_bytes(int64_t n) {
  if (n < 0) n = 0;
  pred_ws w; int64_t total;
  pred_ws_layout(n, &w, nullptr, &total);
  return total;
}

/* Column dtypes and the postfix program, checked on the host before anything
 * is launched: shared by gpuq_filter_expr and gpuq_join_probe_keys_cond
 * (`who` prefixes the messages). The caller has checked ncols and ninsns
 * against the caps. */
static int pred_check_program(const char* who, const gpuq_col* cols, int32_t ncols,
                              const gpuq_pred_insn* prog, int32_t ninsns) {
  for (int c = 0; c < ncols; c++)
    if (cols[c].dtype != GPUQ_INT64 && cols[c].dtype != GPUQ_FLOAT64)
      FAIL(GPUQ_ERR_INVALID, "%s: column %d has unsupported dtype %d", who, c, cols[c].dtype);
  int depth = 0;
  for (int pc = 0; pc < ninsns; pc++) {
    const gpuq_pred_insn& in = prog[pc];
    int pops = 0;
    switch (in.opcode) {
      case GPUQ_PRED_CMP_COL:
        if (in.col_b < 0 || in.col_b >= ncols)
          FAIL(GPUQ_ERR_INVALID, "%s: insn %d: column index %d out of range", who, pc, in.col_b);
        /* fallthrough */
      case GPUQ_PRED_CMP_LIT:
        if (in.cmp < GPUQ_CMP_EQ || in.cmp > GPUQ_CMP_NE)
          FAIL(GPUQ_ERR_INVALID, "%s: insn %d: bad comparison %d", who, pc, in.cmp);
        /* fallthrough */
      case GPUQ_PRED_IS_NULL:
      case GPUQ_PRED_IS_NOT_NULL:
        if (in.col_a < 0 || in.col_a >= ncols)
          FAIL(GPUQ_ERR_INVALID, "%s: insn %d: column index %d out of range", who, pc, in.col_a);
        if (in.opcode == GPUQ_PRED_CMP_COL && cols[in.col_a].dtype != cols[in.col_b].dtype)
          FAIL(GPUQ_ERR_INVALID, "%s: insn %d: column dtypes differ (%d vs %d)", who, pc,
               cols[in.col_a].dtype, cols[in.col_b].dtype);
        break;
      case GPUQ_PRED_CONST:
        if (in.cmp < GPUQ_PRED_FALSE || in.cmp > GPUQ_PRED_NULL)
          FAIL(GPUQ_ERR_INVALID, "%s: insn %d: bad constant %d", who, pc, in.cmp);
        break;
      case GPUQ_PRED_AND:
      case GPUQ_PRED_OR: pops = 2; break;
      case GPUQ_PRED_NOT: pops = 1; break;
      default:
        FAIL(GPUQ_ERR_INVALID, "%s: insn %d: bad opcode %d", who, pc, in.opcode);
    }
    if (depth < pops)
      FAIL(GPUQ_ERR_INVALID, "%s: insn %d: stack underflow", who, pc);
    depth += 1 - pops;
    if (depth > GPUQ_PRED_MAX_DEPTH)
      FAIL(GPUQ_ERR_INVALID, "%s: insn %d: stack depth exceeds %d", who, pc, GPUQ_PRED_MAX_DEPTH);
  }
  if (depth != 1)
    FAIL(GPUQ_ERR_INVALID, "%s: program leaves %d values on the stack, need 1", who, depth);
  return GPUQ_OK;
}

extern "C" int gpuq_filter_expr(void* stream, int64_t n,
                                const gpuq_col* cols, int32_t ncols,
                                const gpuq_pred_insn* prog, int32_t ninsns,
                                uint32_t* out_perm, int64_t* out_count,
                                void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || n > 0xFFFFFFFFLL)
    FAIL(GPUQ_ERR_INVALID, "filter_expr: nrows %lld out of range", (long long)n);
  if (ncols < 0 || ncols > GPUQ_PRED_MAX_COLS)
    FAIL(GPUQ_ERR_INVALID, "filter_expr: %d columns, need 0..%d", ncols, GPUQ_PRED_MAX_COLS);
  if (ninsns < 1 || ninsns > GPUQ_PRED_MAX_INSNS)
    FAIL(GPUQ_ERR_INVALID, "filter_expr: %d instructions, need 1..%d", ninsns, GPUQ_PRED_MAX_INSNS);
  if (int rc = pred_check_program("filter_expr", cols, ncols, prog, ninsns)) return rc;
  pred_args a;
  pred_fill_args(&a, cols, ncols, prog, ninsns);
  pred_ws w; int64_t need;
  pred_ws_layout(n, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "filter_expr: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(out_count, 0, 8, s));
    return GPUQ_OK;
  }
  const int64_t nb = (n + PRED_TILE - 1) / PRED_TILE;
  { hipEvent_t _pe = prof_begin(s);
  k_pred_mask<<<dim3((uint32_t)nb), PRED_BLOCK, 0, s>>>(n, a, w.mask, w.cnt);
  prof_end("filter_expr_mask", s, _pe); }
  HIP_TRY(hipGetLastError());
  { hipEvent_t _pe = prof_begin(s);
  int rc = exclusive_scan_u32(s, nb, w.cnt, w.scan, w.block_sums);
  if (rc) return rc;
  k_pred_emit<<<dim3((uint32_t)nb), PRED_BLOCK, 0, s>>>(
      w.mask, w.scan, (uint32_t)nb, out_perm, (unsigned long long*)out_count);
  prof_end("filter_expr_emit", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ---- composite-key join: residual condition inside the probe ----
 * (gpuq_join_probe_keys_cond; it sits here, not beside k_joink_probe, because
 * it interprets the predicate program defined above.)
 *
 * k_joink_probe with "match" narrowed to "candidate for which the program is
 * TRUE": the skeleton's accept functor evaluates the program on every (probe
 * row, build row) candidate, in phase A and again in phase B's walk past c1.
 *
 * Blocks own JOINC_CHUNK = 1024 rows (4 rounds), not JOIN_CHUNK: the rounds
 * are unrolled so that cnt / c0 / c1 stay in registers, and each round now
 * carries two copies of the interpreter. One cursor atomicAdd per 1024 probe
 * rows is still negligible.
 *
 * The program and the column table arrive by value in the kernel arguments,
 * so the program counter and every column index are wave-uniform even though
 * the lanes of a wave sit at different depths of different chains. A leaf
 * loads its operand for the pair at hand: a build-side column at the build
 * row (one random 8-byte load), a probe-side column at the probe row
 * (coalesced across the wave, and served by the L1 from the row's second
 * candidate on).
 * Holding the probe-side operands of a row in registers instead was tried:
 * with up to GPUQ_PRED_MAX_COLS columns they form an array that a leaf has
 * to pick from by its (uniform, but runtime) column index, which the
 * compiler turns into an indexed private array and parks in LDS — 18 KB per
 * block and an LDS round trip per leaf — so the loads stayed. */
#define JOINC_CHUNK 1024

struct joinc_args {
  pred_args p;
  int32_t side[GPUQ_PRED_MAX_COLS];   /* GPUQ_JOIN_SIDE_* */
};

/* TRUE iff the program evaluates to TRUE for (probe row i, build row b).
 * Column c is read at the row of its side: the side is wave-uniform, the row
 * index a select between two registers. */
DEV bool joinc_pass(const joinc_args& a, int64_t i, unsigned int b) {
  uint32_t tb[1];
  pred_eval<1>(a.p, [&](int c, uint64_t (&v)[1]) {
    const int64_t row = a.side[c] == GPUQ_JOIN_SIDE_BUILD ? (int64_t)b : i;
    v[0] = ((const uint64_t*)a.p.data[c])[row];
    return (uint32_t)bit_valid(a.p.validity[c], row);
  }, tb);
  return tb[0] & 1;
}

/* JT 0-4 as k_joink_probe, with joinc_pass as the accept functor */
template <int JT>
__global__ __launch_bounds__(JOIN_BLOCK)
void k_joink_probe_cond(int64_t n, joink_cols kc, int nkeys, int sw,
                        const unsigned long long* slots, const unsigned int* next,
                        joink_sp* sp, int64_t cap_mask, joinc_args a,
                        uint32_t* out_p, uint32_t* out_b, int64_t out_cap,
                        unsigned long long* matched) {
  constexpr int ROUNDS = JOINC_CHUNK / JOIN_BLOCK;
  const int64_t base = (int64_t)blockIdx.x * JOINC_CHUNK + threadIdx.x;
  auto accept = [&](int64_t i, unsigned int b) { return joinc_pass(a, i, b); };
  uint32_t cnt[ROUNDS];
  unsigned int c0[ROUNDS], c1[ROUNDS];
  uint32_t lane_total = 0;
  #pragma unroll
  for (int r = 0; r < ROUNDS; r++) {
    const int64_t i = base + r * JOIN_BLOCK;
    const unsigned int head =
        i < n ? joink_find_head(kc, nkeys, sw, slots, cap_mask, i) : JOIN_NIL;
    join_collect<JT>(head, i, next, matched, accept, &cnt[r], &c0[r], &c1[r]);
    if (JT == 0) lane_total += cnt[r];
    else if (i < n) lane_total += jt_emit_count(JT, cnt[r]);
  }
  int64_t o = join_reserve(lane_total, &sp->j.cursor);
  #pragma unroll
  for (int r = 0; r < ROUNDS; r++) {
    const int64_t i = base + r * JOIN_BLOCK;
    join_emit_row<JT>(i, i < n, cnt[r], c0[r], c1[r], next, accept, o,
                      out_p, out_b, out_cap);
  }
}

extern "C" int gpuq_join_probe_keys_cond(void* stream, int64_t prows,
                                         const gpuq_col* probe_keys, int32_t nkeys,
                                         void* workspace, int64_t cap, int64_t brows,
                                         int32_t join_type,
                                         const gpuq_col* cond_cols,
                                         const int32_t* cond_sides, int32_t ncond_cols,
                                         const gpuq_pred_insn* prog, int32_t ninsns,
                                         uint32_t* out_p, uint32_t* out_b,
                                         int64_t out_cap, int64_t* out_nmatches) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "join_keys probe_cond";
  if (int rc = joink_check_table(who, nkeys, cap, brows)) return rc;
  if (join_type == 5)
    FAIL(GPUQ_ERR_INVALID, "%s: the null-aware anti join (type 5) takes no "
         "condition", who);
  if (join_type < 0 || join_type > 4)
    FAIL(GPUQ_ERR_INVALID, "%s: bad join_type %d", who, join_type);
  if (prows < 0 || prows > 0xFFFFFFFELL)
    FAIL(GPUQ_ERR_INVALID, "%s: probe rows %lld do not fit 32-bit rowids", who,
         (long long)prows);
  joink_cols kc = {};
  if (int rc = joink_check_cols(who, probe_keys, nkeys, &kc)) return rc;
  if (ncond_cols < 1 || ncond_cols > GPUQ_PRED_MAX_COLS)
    FAIL(GPUQ_ERR_INVALID, "%s: %d condition columns, need 1..%d", who, ncond_cols,
         GPUQ_PRED_MAX_COLS);
  if (!cond_cols) FAIL(GPUQ_ERR_INVALID, "%s: condition columns missing", who);
  if (!cond_sides) FAIL(GPUQ_ERR_INVALID, "%s: condition sides missing", who);
  if (!prog) FAIL(GPUQ_ERR_INVALID, "%s: condition program missing", who);
  for (int c = 0; c < ncond_cols; c++)
    if (cond_sides[c] != GPUQ_JOIN_SIDE_PROBE && cond_sides[c] != GPUQ_JOIN_SIDE_BUILD)
      FAIL(GPUQ_ERR_INVALID, "%s: condition column %d has side %d, need 0 (probe) "
           "or 1 (build)", who, c, cond_sides[c]);
  if (ninsns < 1 || ninsns > GPUQ_PRED_MAX_INSNS)
    FAIL(GPUQ_ERR_INVALID, "%s: %d instructions, need 1..%d", who, ninsns,
         GPUQ_PRED_MAX_INSNS);
  if (int rc = pred_check_program(who, cond_cols, ncond_cols, prog, ninsns)) return rc;
  joinc_args a;
  pred_fill_args(&a.p, cond_cols, ncond_cols, prog, ninsns);
  memset(a.side, 0, sizeof(a.side));
  for (int c = 0; c < ncond_cols; c++) a.side[c] = cond_sides[c];
  joink_ws w; int64_t need;
  joink_ws_layout(cap, brows, nkeys, &w, (char*)workspace, &need);
  int sw = joink_stride_words(nkeys);
  dim3 jg((uint32_t)((prows + JOINC_CHUNK - 1) / JOINC_CHUNK));
  if (int rc = join_launch_probe<4>(s, &w.sp->j, prows, join_type, "join_keys_probe_cond", [&](auto jt) {
        k_joink_probe_cond<decltype(jt)::value><<<jg, JOIN_BLOCK, 0, s>>>(
            prows, kc, nkeys, sw, w.slots, w.next, w.sp, cap - 1, a, out_p,
            out_b, out_cap, w.matched);
      })) return rc;
  return join_read_count(s, &w.sp->j, who, "matches", out_cap, out_nmatches);
}

/* One int64 operation with Java long semantics (Spark non-ANSI): + - * wrap
 * modulo 2^64, done in uint64_t because signed overflow is undefined in C++;
 * / truncates toward zero and INT64_MIN / -1 == INT64_MIN (divisor -1 is an
 * unsigned negation; the signed quotient would overflow). The caller rules
 * out a zero divisor. */
template <int OP>
DEV int64_t binop_i64(int64_t x, int64_t y) {
  uint64_t ux = (uint64_t)x, uy = (uint64_t)y;
  if (OP == 0) return (int64_t)(ux + uy);
  if (OP == 1) return (int64_t)(ux - uy);
  if (OP == 2) return (int64_t)(ux * uy);
  if (OP == 4) return (int64_t)(uy - ux);
  if (y == -1) return (int64_t)(0 - ux);
  return x / y;
}

template <int OP>
DEV double binop_f64(double x, double y) {
  return OP == 0 ? x + y : OP == 1 ? x - y : OP == 2 ? x * y
         : OP == 4 ? y - x : x / y;
}

/* out = a OP b (b = column or broadcast literal), no NULL tracking: the
 * caller owns validity (AVG = sum / count fixes it from the count). An
 * integral zero divisor yields 0 here. */
template <int DTYPE, int OP, bool B_IS_LIT>
__global__ void k_project_binop(int64_t n, const void* a, const void* b,
                                double lit_f, int64_t lit_i, void* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    if (DTYPE == GPUQ_FLOAT64) {
      double x = ((const double*)a)[i];
      double y = B_IS_LIT ? lit_f : ((const double*)b)[i];
      ((double*)out)[i] = binop_f64<OP>(x, y);
    } else {
      int64_t x = ((const int64_t*)a)[i];
      int64_t y = B_IS_LIT ? lit_i : ((const int64_t*)b)[i];
      ((int64_t*)out)[i] = (OP == 3 && y == 0) ? 0 : binop_i64<OP>(x, y);
    }
  }
}

/* NULL-aware form: the output row is valid iff both inputs are valid and the
 * op is not a division by zero (Spark non-ANSI Divide: x / 0 is NULL; for
 * float64 -0.0 is a zero too). NULL output rows hold 0, never the bytes that
 * sat under an input NULL.
 * One thread per row, so loads and stores coalesce like the plain kernel's.
 * A wavefront covers 64 consecutive rows starting at a multiple of 64 (block
 * and grid stride are multiples of 64), i.e. exactly 8 bitmap bytes: the
 * lanes' valid bits are collected with one ballot and every 8th lane stores
 * its byte, so no two threads write the same byte and no atomics are needed.
 * The loop bound is wave-uniform (all 64 lanes reach the ballot); lanes past
 * n vote 0, which also zeroes the spare bits of the last byte. */
template <int DTYPE, int OP, bool B_IS_LIT>
__global__ void k_project_binop_nullable(int64_t n, const void* a,
                                         const uint8_t* a_valid, const void* b,
                                         const uint8_t* b_valid, double lit_f,
                                         int64_t lit_i, void* out,
                                         uint8_t* out_bits) {
  int lane = threadIdx.x & 63;
  int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane);
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; base < n; base += stride) {
    int64_t i = base + lane;
    bool ok = i < n;
    if (ok) {
      ok = bit_valid(a_valid, i) && (B_IS_LIT || bit_valid(b_valid, i));
      if (DTYPE == GPUQ_FLOAT64) {
        double x = ((const double*)a)[i];
        double y = B_IS_LIT ? lit_f : ((const double*)b)[i];
        if (OP == 3 && y == 0.0) ok = false;
        ((double*)out)[i] = ok ? binop_f64<OP>(x, y) : 0.0;
      } else {
        int64_t x = ((const int64_t*)a)[i];
        int64_t y = B_IS_LIT ? lit_i : ((const int64_t*)b)[i];
        if (OP == 3 && y == 0) ok = false;
        ((int64_t*)out)[i] = ok ? binop_i64<OP>(x, y) : 0;
      }
    }
    uint64_t m = __ballot(ok);
    if ((lane & 7) == 0 && i < n) out_bits[i >> 3] = (uint8_t)(m >> lane);
  }
}

extern "C" int gpuq_project_binop(void* stream, int64_t n, gpuq_col a,
                                  const void* b /* col data or NULL */,
                                  double lit_f, int64_t lit_i, int32_t op,
                                  void* out) {
  hipStream_t s = (hipStream_t)stream;
  if (op < 0 || op > 4) FAIL(GPUQ_ERR_INVALID, "project: bad op %d", op);
  if (a.validity)
    FAIL(GPUQ_ERR_INVALID, "project: validity needs gpuq_project_binop_nullable");
  dim3 g = grid1d(n);
#define PJ(DT, OPV) do { \
    if (b) k_project_binop<DT, OPV, false><<<g, 256, 0, s>>>(n, a.data, b, lit_f, lit_i, out); \
    else   k_project_binop<DT, OPV, true><<<g, 256, 0, s>>>(n, a.data, b, lit_f, lit_i, out); \
  } while (0)
  if (a.dtype == GPUQ_FLOAT64) {
    if (op == 0) PJ(GPUQ_FLOAT64, 0); else if (op == 1) PJ(GPUQ_FLOAT64, 1);
    else if (op == 2) PJ(GPUQ_FLOAT64, 2); else if (op == 4) PJ(GPUQ_FLOAT64, 4);
    else PJ(GPUQ_FLOAT64, 3);
  } else if (a.dtype == GPUQ_INT64) {
    if (op == 0) PJ(GPUQ_INT64, 0); else if (op == 1) PJ(GPUQ_INT64, 1);
    else if (op == 2) PJ(GPUQ_INT64, 2); else if (op == 4) PJ(GPUQ_INT64, 4);
    else PJ(GPUQ_INT64, 3);
  } else {
    FAIL(GPUQ_ERR_INVALID, "project: unsupported dtype %d", a.dtype);
  }
#undef PJ
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

extern "C" int gpuq_project_binop_nullable(void* stream, int64_t n, gpuq_col a,
                                           gpuq_col b /* data NULL => literal */,
                                           double lit_f, int64_t lit_i,
                                           int32_t op, void* out,
                                           uint8_t* out_bits) {
  hipStream_t s = (hipStream_t)stream;
  if (op < 0 || op > 4) FAIL(GPUQ_ERR_INVALID, "project: bad op %d", op);
  if (a.dtype != GPUQ_FLOAT64 && a.dtype != GPUQ_INT64)
    FAIL(GPUQ_ERR_INVALID, "project: unsupported dtype %d", a.dtype);
  if (b.data && b.dtype != a.dtype)
    FAIL(GPUQ_ERR_INVALID, "project: operand dtypes differ (%d vs %d)",
         a.dtype, b.dtype);
  if (!b.data && b.validity)
    FAIL(GPUQ_ERR_INVALID, "project: a literal operand has no validity");
  if (n == 0) return GPUQ_OK;   /* an empty bitmap's pointer may be NULL */
  if (!out_bits) {
    /* nothing can be NULL: the plain kernel */
    if (a.validity || b.validity || op == GPUQ_BINOP_DIV)
      FAIL(GPUQ_ERR_INVALID,
           "project: nullable inputs and '/' need an output bitmap");
    return gpuq_project_binop(stream, n, a, b.data, lit_f, lit_i, op, out);
  }
  dim3 g = grid1d(n);   /* 256-thread blocks: whole wavefronts */
#define PJN(DT, OPV) do { \
    if (b.data) k_project_binop_nullable<DT, OPV, false><<<g, 256, 0, s>>>( \
        n, a.data, a.validity, b.data, b.validity, lit_f, lit_i, out, out_bits); \
    else k_project_binop_nullable<DT, OPV, true><<<g, 256, 0, s>>>( \
        n, a.data, a.validity, b.data, b.validity, lit_f, lit_i, out, out_bits); \
  } while (0)
#define PJN_OPS(DT) do { \
    if (op == 0) PJN(DT, 0); else if (op == 1) PJN(DT, 1); \
    else if (op == 2) PJN(DT, 2); else if (op == 4) PJN(DT, 4); \
    else PJN(DT, 3); \
  } while (0)
  if (a.dtype == GPUQ_FLOAT64) PJN_OPS(GPUQ_FLOAT64);
  else PJN_OPS(GPUQ_INT64);
#undef PJN_OPS
#undef PJN
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ---- compound expressions: one fused pass (gpuq_project_expr) ----
 *
 * k_expr_eval has k_pred_mask's shape: one block per EXPR_TILE rows, row r of
 * thread t is tile + r * EXPR_BLOCK + t, instructions outer and the rows
 * inner and unrolled (a COL issues its loads back to back), the program and
 * the column / output tables by value in the kernel arguments. The program
 * counter, the opcode, the dtype and the stack depth are the same in every
 * lane, so every branch of the interpreter is wave-uniform.
 *
 * The value stack lives in registers as a shifting stack of named slots:
 * slot 0 is the top, a push moves every slot one down, a pop one up, and every
 * operand sits at a fixed slot (a binary op reads slots 1 and 0), so nothing
 * is indexed by a runtime value. The host's stack simulation knows the depth
 * in front of every instruction and leaves it in the instruction's pad word;
 * while the depth stays within EXPR_SHALLOW only that many slots move (a
 * wave-uniform branch), which is what Q1-sized programs pay. NULL flags are
 * bit d of one word per row and shift with the slots. The compiler
 * structurizes this loop
 * although its branches are uniform, and the joins keep two copies of the
 * stack alive, so registers go with the slot count: hence the 4-slot kernel
 * beside the 8-slot one, and 4 rows per thread (compile table in DESIGN.md).
 *
 * OUT stores the value (0 under a NULL), ballots the valid flags — a wave
 * covers 64 consecutive rows from a multiple of 64, i.e. 8 whole bitmap bytes,
 * every 8th lane stores its byte, no atomics; tiles are multiples of 64 rows
 * so no two blocks share a byte — and keeps the row's NULL flag for REF. REF
 * re-reads the value its own thread stored.
 */
#define EXPR_BLOCK 256
#define EXPR_ITEMS 4
#define EXPR_TILE (EXPR_BLOCK * EXPR_ITEMS)   /* 1024 rows per block */
#define EXPR_SHALLOW 4    /* slots of the small kernel and of the cheap shifts */

struct expr_args {
  const void* data[GPUQ_EXPR_MAX_COLS];
  const uint8_t* validity[GPUQ_EXPR_MAX_COLS];
  void* out[GPUQ_EXPR_MAX_OUTS];
  uint8_t* out_bits[GPUQ_EXPR_MAX_OUTS];
  int32_t ninsns;
  gpuq_expr_insn insn[GPUQ_EXPR_MAX_INSNS];   /* pad = stack depth in front */
};

template <int DEPTH>
struct expr_regs {
  uint64_t v[DEPTH][EXPR_ITEMS];
  uint32_t nl[EXPR_ITEMS];      /* bit d: slot d is NULL */
  uint32_t onull[EXPR_ITEMS];   /* bit k: OUT k wrote a NULL */
};

DEV double expr_f(uint64_t x) { return __longlong_as_double((long long)x); }
DEV uint64_t expr_u(double x) { return (uint64_t)__double_as_longlong(x); }

/* Java's (long) d, without a branch: NaN becomes 0, the value is clamped to
 * [-2^63, 2^63 - 1024] (the largest double below 2^63) so the conversion is
 * defined, and what was at or beyond 2^63 then reads INT64_MAX; -2^63 and
 * below convert to INT64_MIN by the clamp itself. */
DEV int64_t expr_f64_to_i64(double d) {
  double c = d != d ? 0.0 : d;
  c = fmax(fmin(c, 9223372036854774784.0), -9223372036854775808.0);
  int64_t t = (int64_t)c;
  return d >= 9223372036854775808.0 ? INT64_MAX : t;
}

/* filter_cmp_f64's truth table (total order, -0.0 == 0.0, NaN == NaN and
 * greatest) without its divergent branch on NaN: op is wave-uniform here, so
 * this leaves no lane-dependent control flow in the interpreter loop. */
DEV bool expr_cmp_f64(double x, int op, double y) {
  const bool xn = x != x, yn = y != y;
  const bool eq = (xn & yn) | (x == y);
  const bool lt = !xn & (yn | (x < y));
  switch (op) {
    case GPUQ_CMP_EQ: return eq;
    case GPUQ_CMP_LT: return lt;
    case GPUQ_CMP_LE: return lt | eq;
    case GPUQ_CMP_GT: return !(lt | eq);
    case GPUQ_CMP_GE: return !lt;
    default: return !eq;
  }
}

#define EXPR_ROWS _Pragma("unroll") for (int r = 0; r < EXPR_ITEMS; r++)
#define EXPR_NL(d) ((s.nl[r] >> (d)) & 1u)
#define EXPR_SET_NL(d, x) s.nl[r] = (s.nl[r] & ~(1u << (d))) | ((uint32_t)(x) << (d))

/* make room on top: slot d-1 moves to slot d for d = LAST .. 1 */
template <int LAST, typename REGS>
DEV void expr_shift_down(REGS& s) {
  #pragma unroll
  for (int d = LAST; d >= 1; d--) { EXPR_ROWS s.v[d][r] = s.v[d - 1][r]; }
  EXPR_ROWS s.nl[r] <<= 1;
}

/* drop the BY top slots: slot d+BY moves to slot d for d = 0 .. LAST */
template <int BY, int LAST, typename REGS>
DEV void expr_drop(REGS& s) {
  #pragma unroll
  for (int d = 0; d <= LAST; d++) { EXPR_ROWS s.v[d][r] = s.v[d + BY][r]; }
  EXPR_ROWS s.nl[r] >>= BY;
}

/* a OP b on slots 1 and 0 into slot 1, the operator and type fixed at compile
 * time so the row loop holds no dispatch */
template <int OP, bool F64, typename REGS>
DEV void expr_arith(REGS& s) {
  EXPR_ROWS {
    const uint64_t x = s.v[1][r], y = s.v[0][r];
    s.v[1][r] = F64 ? expr_u(binop_f64<OP>(expr_f(x), expr_f(y)))
                    : (uint64_t)binop_i64<OP>((int64_t)x, (int64_t)y);
    EXPR_SET_NL(1, EXPR_NL(1) | EXPR_NL(0));
  }
}

template <int OP, bool F64, typename REGS>
DEV void expr_cmp(REGS& s) {
  EXPR_ROWS {
    const bool t = F64
        ? expr_cmp_f64(expr_f(s.v[1][r]), OP, expr_f(s.v[0][r]))
        : filter_cmp_i64((int64_t)s.v[1][r], OP, (int64_t)s.v[0][r]);
    s.v[1][r] = t ? 1 : 0;
    EXPR_SET_NL(1, EXPR_NL(1) | EXPR_NL(0));
  }
}

#define EXPR_BY_TYPE(FN, OP) do { \
    if (f64) FN<OP, true>(s); else FN<OP, false>(s); } while (0)

/* One instruction with `depth` values on the stack in front of it. FULL: every
 * row of the block's tile is below n, so no load or store is predicated (no
 * exec-mask branch around them; only the int64 divide keeps lane-dependent
 * branches of its own). In a full tile all eight lanes of a bitmap byte store
 * it, with the same value. */
template <bool FULL, int DEPTH>
DEV void expr_step(expr_regs<DEPTH>& s, const expr_args& a, const int pc,
                   const int64_t n, const int64_t base, const int lane) {
  const int depth = a.insn[pc].pad;
  const int opcode = a.insn[pc].opcode;
  const int arg = a.insn[pc].arg;
  const bool f64 = a.insn[pc].dtype == GPUQ_FLOAT64;
  if (opcode <= GPUQ_EXPR_REF) {
    {
      constexpr int D = 0;   /* the new top */
      if (DEPTH == EXPR_SHALLOW || depth < EXPR_SHALLOW) expr_shift_down<EXPR_SHALLOW - 1>(s);
      else expr_shift_down<DEPTH - 1>(s);
      if (opcode == GPUQ_EXPR_COL) {
        const uint64_t* d = (const uint64_t*)a.data[arg];
        const uint8_t* v = a.validity[arg];
        EXPR_ROWS {
          int64_t i = base + r * EXPR_BLOCK;
          bool in = FULL || i < n;
          s.v[D][r] = in ? d[i] : 0;
          EXPR_SET_NL(D, !(in && bit_valid(v, i)));
        }
      } else if (opcode == GPUQ_EXPR_LIT) {
        const uint64_t lit = f64 ? expr_u(a.insn[pc].lit_f64)
                                 : (uint64_t)a.insn[pc].lit_i64;
        const uint32_t isnull = arg != 0;
        EXPR_ROWS { s.v[D][r] = lit; EXPR_SET_NL(D, isnull); }
      } else {   /* REF: what this thread stored for OUT arg */
        const uint64_t* o = (const uint64_t*)a.out[arg];
        EXPR_ROWS {
          int64_t i = base + r * EXPR_BLOCK;
          s.v[D][r] = FULL || i < n ? o[i] : 0;
          EXPR_SET_NL(D, (s.onull[r] >> arg) & 1u);
        }
      }
    }
  } else if (opcode == GPUQ_EXPR_ARITH || opcode == GPUQ_EXPR_CMP ||
             opcode == GPUQ_EXPR_AND || opcode == GPUQ_EXPR_OR ||
             opcode == GPUQ_EXPR_COALESCE) {
    {
      constexpr int A = 1, B = 0;   /* the result replaces a, then b is dropped */
      if (opcode == GPUQ_EXPR_ARITH && arg == GPUQ_BINOP_DIV) {
        /* the divide expansions are long: one row at a time (the barrier
         * keeps the scheduler from interleaving the rows), or their
         * temporaries set the kernel's register count */
        if (f64) {
          EXPR_ROWS {
            const double fy = expr_f(s.v[B][r]);
            s.v[A][r] = expr_u(binop_f64<3>(expr_f(s.v[A][r]), fy));
            EXPR_SET_NL(A, EXPR_NL(A) | EXPR_NL(B) | (uint32_t)(fy == 0.0));
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          EXPR_ROWS {
            const int64_t iy = (int64_t)s.v[B][r];
            /* a zero divisor (also under a NULL) divides by 1: no trap, and
             * the row is NULL anyway */
            s.v[A][r] = (uint64_t)binop_i64<3>((int64_t)s.v[A][r], iy == 0 ? 1 : iy);
            EXPR_SET_NL(A, EXPR_NL(A) | EXPR_NL(B) | (uint32_t)(iy == 0));
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else if (opcode == GPUQ_EXPR_ARITH) {
        if (arg == GPUQ_BINOP_ADD) EXPR_BY_TYPE(expr_arith, GPUQ_BINOP_ADD);
        else if (arg == GPUQ_BINOP_SUB) EXPR_BY_TYPE(expr_arith, GPUQ_BINOP_SUB);
        else EXPR_BY_TYPE(expr_arith, GPUQ_BINOP_MUL);
      } else if (opcode == GPUQ_EXPR_CMP) {
        switch (arg) {
          case GPUQ_CMP_EQ: EXPR_BY_TYPE(expr_cmp, GPUQ_CMP_EQ); break;
          case GPUQ_CMP_LT: EXPR_BY_TYPE(expr_cmp, GPUQ_CMP_LT); break;
          case GPUQ_CMP_LE: EXPR_BY_TYPE(expr_cmp, GPUQ_CMP_LE); break;
          case GPUQ_CMP_GT: EXPR_BY_TYPE(expr_cmp, GPUQ_CMP_GT); break;
          case GPUQ_CMP_GE: EXPR_BY_TYPE(expr_cmp, GPUQ_CMP_GE); break;
          default: EXPR_BY_TYPE(expr_cmp, GPUQ_CMP_NE); break;
        }
      } else if (opcode == GPUQ_EXPR_COALESCE) {
        EXPR_ROWS {
          const uint32_t an = EXPR_NL(A);
          s.v[A][r] = an ? s.v[B][r] : s.v[A][r];
          EXPR_SET_NL(A, an & EXPR_NL(B));
        }
      } else {   /* AND / OR: the deciding value (FALSE / TRUE) wins over NULL */
        const uint32_t win = opcode == GPUQ_EXPR_OR ? 1u : 0u;
        EXPR_ROWS {
          uint32_t an = EXPR_NL(A), bn = EXPR_NL(B);
          uint32_t aw = !an && ((uint32_t)s.v[A][r] & 1u) == win;
          uint32_t bw = !bn && ((uint32_t)s.v[B][r] & 1u) == win;
          uint32_t decided = aw | bw;
          s.v[A][r] = decided ? win : (win ^ 1u);
          EXPR_SET_NL(A, !decided && (an | bn));
        }
      }
      if (DEPTH == EXPR_SHALLOW || depth <= EXPR_SHALLOW) expr_drop<1, EXPR_SHALLOW - 2>(s);
      else expr_drop<1, DEPTH - 2>(s);
    }
  } else if (opcode == GPUQ_EXPR_SELECT) {
    constexpr int E = 2, T = 1, C = 0;
    EXPR_ROWS {
      const bool take = (EXPR_NL(C) == 0u) & ((s.v[C][r] & 1u) != 0u);
      s.v[E][r] = take ? s.v[T][r] : s.v[E][r];
      EXPR_SET_NL(E, take ? EXPR_NL(T) : EXPR_NL(E));
    }
    if (DEPTH == EXPR_SHALLOW || depth <= EXPR_SHALLOW) expr_drop<2, EXPR_SHALLOW - 3>(s);
    else expr_drop<2, DEPTH - 3>(s);
  } else {   /* one operand on top */
    {
      constexpr int A = 0;
      if (opcode == GPUQ_EXPR_NEG) {
        if (f64) { EXPR_ROWS s.v[A][r] ^= SIGNBIT; }
        else { EXPR_ROWS s.v[A][r] = 0ULL - s.v[A][r]; }
      } else if (opcode == GPUQ_EXPR_ABS) {
        if (f64) { EXPR_ROWS s.v[A][r] &= ~SIGNBIT; }
        else {
          EXPR_ROWS {
            const uint64_t x = s.v[A][r];
            s.v[A][r] = (int64_t)x < 0 ? 0ULL - x : x;
          }
        }
      } else if (opcode == GPUQ_EXPR_CAST) {
        /* dtype is the source: f64 -> i64, else i64 -> f64 or BOOL -> i64 */
        if (f64) {
          EXPR_ROWS {
            s.v[A][r] = (uint64_t)expr_f64_to_i64(expr_f(s.v[A][r]));
            __builtin_amdgcn_sched_barrier(0);
          }
        } else if (arg == GPUQ_FLOAT64) {
          EXPR_ROWS s.v[A][r] = expr_u((double)(int64_t)s.v[A][r]);
        } else {
          EXPR_ROWS s.v[A][r] &= 1u;
        }
      } else if (opcode == GPUQ_EXPR_IS_NULL || opcode == GPUQ_EXPR_IS_NOT_NULL) {
        const uint32_t flip = opcode == GPUQ_EXPR_IS_NOT_NULL ? 1u : 0u;
        EXPR_ROWS { s.v[A][r] = EXPR_NL(A) ^ flip; EXPR_SET_NL(A, 0u); }
      } else if (opcode == GPUQ_EXPR_NOT) {
        EXPR_ROWS s.v[A][r] = (s.v[A][r] & 1u) ^ 1u;
      } else {   /* OUT */
        uint64_t* o = (uint64_t*)a.out[arg];
        uint8_t* bits = a.out_bits[arg];
        EXPR_ROWS {
          int64_t i = base + r * EXPR_BLOCK;
          bool in = FULL || i < n;
          uint32_t nul = EXPR_NL(A);
          if (in) o[i] = nul ? 0 : s.v[A][r];
          s.onull[r] = (s.onull[r] & ~(1u << arg)) | (nul << arg);
          if (bits) {   /* wave-uniform: all 64 lanes reach the ballot */
            unsigned long long m = __ballot(in && !nul);
            if (FULL || ((lane & 7) == 0 && in)) bits[i >> 3] = (uint8_t)(m >> (lane & ~7));
          }
        }
        if (DEPTH == EXPR_SHALLOW || depth <= EXPR_SHALLOW) expr_drop<1, EXPR_SHALLOW - 2>(s);
        else expr_drop<1, DEPTH - 2>(s);
      }
    }
  }
}

template <bool FULL, int DEPTH>
DEV void expr_run(const int64_t n, const expr_args& a) {
  const int64_t base = (int64_t)blockIdx.x * EXPR_TILE + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  expr_regs<DEPTH> s;
  #pragma unroll
  for (int r = 0; r < EXPR_ITEMS; r++) {
    #pragma unroll
    for (int d = 0; d < DEPTH; d++) s.v[d][r] = 0;
    s.nl[r] = 0; s.onull[r] = 0;
  }
  for (int pc = 0; pc < a.ninsns; pc++) expr_step<FULL, DEPTH>(s, a, pc, n, base, lane);
}

/* DEPTH slots: the host picks the EXPR_SHALLOW-slot kernel for a program whose
 * stack never grows past it (Q1's needs 3), which halves the registers */
template <int DEPTH>
__global__ __launch_bounds__(EXPR_BLOCK)
void k_expr_eval(int64_t n, expr_args a) {
  if ((int64_t)(blockIdx.x + 1) * EXPR_TILE <= n) expr_run<true, DEPTH>(n, a);
  else expr_run<false, DEPTH>(n, a);
}
#undef EXPR_BY_TYPE
#undef EXPR_ROWS
#undef EXPR_NL
#undef EXPR_SET_NL

static const char* expr_type_name(int t) {
  return t == GPUQ_INT64 ? "int64" : t == GPUQ_FLOAT64 ? "float64"
         : t == GPUQ_EXPR_BOOL ? "bool" : "?";
}

extern "C" int gpuq_project_expr(void* stream, int64_t n,
                                 const gpuq_col* cols, int32_t ncols,
                                 const gpuq_expr_insn* prog, int32_t ninsns,
                                 void* const* outs, uint8_t* const* out_bits,
                                 const int32_t* out_dtypes, int32_t nouts) {
  hipStream_t s = (hipStream_t)stream;
#define XFAIL(...) FAIL(GPUQ_ERR_INVALID, "project_expr: " __VA_ARGS__)
  if (n < 0 || n > 0xFFFFFFFFLL) XFAIL("nrows %lld out of range", (long long)n);
  if (ncols < 0 || ncols > GPUQ_EXPR_MAX_COLS)
    XFAIL("%d columns, need 0..%d", ncols, GPUQ_EXPR_MAX_COLS);
  if (ninsns < 1 || ninsns > GPUQ_EXPR_MAX_INSNS)
    XFAIL("%d instructions, need 1..%d", ninsns, GPUQ_EXPR_MAX_INSNS);
  if (nouts < 1 || nouts > GPUQ_EXPR_MAX_OUTS)
    XFAIL("%d outputs, need 1..%d", nouts, GPUQ_EXPR_MAX_OUTS);
  if ((ncols && !cols) || !prog || !outs || !out_dtypes)
    XFAIL("missing argument array");
  expr_args a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < ncols; c++) {
    if (cols[c].dtype != GPUQ_INT64 && cols[c].dtype != GPUQ_FLOAT64)
      XFAIL("column %d has unsupported dtype %d", c, cols[c].dtype);
    a.data[c] = cols[c].data;
    a.validity[c] = cols[c].validity;
  }
  for (int k = 0; k < nouts; k++) {
    if (out_dtypes[k] != GPUQ_INT64 && out_dtypes[k] != GPUQ_FLOAT64)
      XFAIL("output %d has unsupported dtype %d", k, out_dtypes[k]);
    a.out[k] = outs[k];
    a.out_bits[k] = out_bits ? out_bits[k] : nullptr;
  }
  int ty[GPUQ_EXPR_MAX_DEPTH];
  bool written[GPUQ_EXPR_MAX_OUTS] = {false, false, false, false};
  int depth = 0, peak = 0;
  for (int pc = 0; pc < ninsns; pc++) {
    const gpuq_expr_insn& in = prog[pc];
    const int dt = in.dtype;
    int pops, push = -1;   /* push: the type pushed, -1 for none */
    switch (in.opcode) {
      case GPUQ_EXPR_COL: case GPUQ_EXPR_LIT: case GPUQ_EXPR_REF: pops = 0; break;
      case GPUQ_EXPR_ARITH: case GPUQ_EXPR_CMP: case GPUQ_EXPR_AND:
      case GPUQ_EXPR_OR: case GPUQ_EXPR_COALESCE: pops = 2; break;
      case GPUQ_EXPR_SELECT: pops = 3; break;
      case GPUQ_EXPR_NEG: case GPUQ_EXPR_ABS: case GPUQ_EXPR_CAST:
      case GPUQ_EXPR_IS_NULL: case GPUQ_EXPR_IS_NOT_NULL: case GPUQ_EXPR_NOT:
      case GPUQ_EXPR_OUT: pops = 1; break;
      default: XFAIL("insn %d: bad opcode %d", pc, in.opcode);
    }
    if (depth < pops) XFAIL("insn %d: stack underflow", pc);
    if (dt != GPUQ_INT64 && dt != GPUQ_FLOAT64 && dt != GPUQ_EXPR_BOOL)
      XFAIL("insn %d: bad dtype %d", pc, dt);
    const int top = pops >= 1 ? ty[depth - 1] : -1;
    const int below = pops >= 2 ? ty[depth - 2] : -1;
    const bool numeric = dt != GPUQ_EXPR_BOOL;
    switch (in.opcode) {
      case GPUQ_EXPR_COL:
        if (in.arg < 0 || in.arg >= ncols)
          XFAIL("insn %d: column index %d out of range", pc, in.arg);
        if (dt != cols[in.arg].dtype)
          XFAIL("insn %d: declared dtype %s, column %d is %s", pc,
                expr_type_name(dt), in.arg, expr_type_name(cols[in.arg].dtype));
        push = dt;
        break;
      case GPUQ_EXPR_LIT:
        if (in.arg != 0 && in.arg != 1)
          XFAIL("insn %d: bad NULL-literal flag %d", pc, in.arg);
        if (dt == GPUQ_EXPR_BOOL && in.arg == 0 && in.lit_i64 != 0 && in.lit_i64 != 1)
          XFAIL("insn %d: bad bool literal %lld", pc, (long long)in.lit_i64);
        push = dt;
        break;
      case GPUQ_EXPR_REF:
        if (in.arg < 0 || in.arg >= nouts)
          XFAIL("insn %d: output index %d out of range", pc, in.arg);
        if (!written[in.arg])
          XFAIL("insn %d: REF to output %d, which is not yet written", pc, in.arg);
        if (dt != out_dtypes[in.arg])
          XFAIL("insn %d: declared dtype %s, output %d is %s", pc,
                expr_type_name(dt), in.arg, expr_type_name(out_dtypes[in.arg]));
        push = dt;
        break;
      case GPUQ_EXPR_ARITH:
      case GPUQ_EXPR_CMP:
        if (in.opcode == GPUQ_EXPR_ARITH && (in.arg < GPUQ_BINOP_ADD || in.arg > GPUQ_BINOP_DIV))
          XFAIL("insn %d: bad binop %d", pc, in.arg);
        if (in.opcode == GPUQ_EXPR_CMP && (in.arg < GPUQ_CMP_EQ || in.arg > GPUQ_CMP_NE))
          XFAIL("insn %d: bad comparison %d", pc, in.arg);
        if (top != below)
          XFAIL("insn %d: operand types differ (%s vs %s)", pc,
                expr_type_name(below), expr_type_name(top));
        if (top == GPUQ_EXPR_BOOL) XFAIL("insn %d: bool operand to an arithmetic or comparison op", pc);
        if (dt != top)
          XFAIL("insn %d: declared dtype %s, operands are %s", pc,
                expr_type_name(dt), expr_type_name(top));
        push = in.opcode == GPUQ_EXPR_CMP ? GPUQ_EXPR_BOOL : dt;
        break;
      case GPUQ_EXPR_NEG:
      case GPUQ_EXPR_ABS:
        if (top == GPUQ_EXPR_BOOL) XFAIL("insn %d: bool operand to an arithmetic or comparison op", pc);
        if (dt != top)
          XFAIL("insn %d: declared dtype %s, operand is %s", pc,
                expr_type_name(dt), expr_type_name(top));
        push = dt;
        break;
      case GPUQ_EXPR_CAST:
        if (!((dt == GPUQ_INT64 && in.arg == GPUQ_FLOAT64) ||
              (dt == GPUQ_FLOAT64 && in.arg == GPUQ_INT64) ||
              (dt == GPUQ_EXPR_BOOL && in.arg == GPUQ_INT64)))
          XFAIL("insn %d: bad cast %s -> %s", pc, expr_type_name(dt), expr_type_name(in.arg));
        if (dt != top)
          XFAIL("insn %d: declared dtype %s, operand is %s", pc,
                expr_type_name(dt), expr_type_name(top));
        push = in.arg;
        break;
      case GPUQ_EXPR_IS_NULL:
      case GPUQ_EXPR_IS_NOT_NULL:
        if (dt != top)
          XFAIL("insn %d: declared dtype %s, operand is %s", pc,
                expr_type_name(dt), expr_type_name(top));
        push = GPUQ_EXPR_BOOL;
        break;
      case GPUQ_EXPR_AND:
      case GPUQ_EXPR_OR:
        if (top != GPUQ_EXPR_BOOL || below != GPUQ_EXPR_BOOL)
          XFAIL("insn %d: non-bool operand to AND / OR", pc);
        if (numeric) XFAIL("insn %d: declared dtype %s, operands are bool", pc, expr_type_name(dt));
        push = GPUQ_EXPR_BOOL;
        break;
      case GPUQ_EXPR_NOT:
        if (top != GPUQ_EXPR_BOOL) XFAIL("insn %d: non-bool operand to NOT", pc);
        if (numeric) XFAIL("insn %d: declared dtype %s, operand is bool", pc, expr_type_name(dt));
        push = GPUQ_EXPR_BOOL;
        break;
      case GPUQ_EXPR_SELECT:
        if (top != GPUQ_EXPR_BOOL) XFAIL("insn %d: non-bool SELECT condition", pc);
        if (below != ty[depth - 3])
          XFAIL("insn %d: operand types differ (%s vs %s)", pc,
                expr_type_name(ty[depth - 3]), expr_type_name(below));
        if (dt != below)
          XFAIL("insn %d: declared dtype %s, operands are %s", pc,
                expr_type_name(dt), expr_type_name(below));
        push = dt;
        break;
      case GPUQ_EXPR_COALESCE:
        if (top != below)
          XFAIL("insn %d: operand types differ (%s vs %s)", pc,
                expr_type_name(below), expr_type_name(top));
        if (dt != top)
          XFAIL("insn %d: declared dtype %s, operands are %s", pc,
                expr_type_name(dt), expr_type_name(top));
        push = dt;
        break;
      default:   /* OUT */
        if (in.arg < 0 || in.arg >= nouts)
          XFAIL("insn %d: output index %d out of range", pc, in.arg);
        if (written[in.arg]) XFAIL("insn %d: output %d written twice", pc, in.arg);
        if (top == GPUQ_EXPR_BOOL) XFAIL("insn %d: bool operand to OUT (cast it to int64)", pc);
        if (dt != top || dt != out_dtypes[in.arg])
          XFAIL("insn %d: declared dtype %s, operand is %s, output %d is %s", pc,
                expr_type_name(dt), expr_type_name(top), in.arg,
                expr_type_name(out_dtypes[in.arg]));
        written[in.arg] = true;
        break;
    }
    a.insn[pc] = in;
    a.insn[pc].pad = depth;
    depth -= pops;
    if (push >= 0) {
      if (depth >= GPUQ_EXPR_MAX_DEPTH)
        XFAIL("insn %d: stack depth exceeds %d", pc, GPUQ_EXPR_MAX_DEPTH);
      ty[depth++] = push;
      if (depth > peak) peak = depth;
    }
  }
  if (depth != 0) XFAIL("program leaves %d values on the stack, need 0", depth);
  for (int k = 0; k < nouts; k++)
    if (!written[k]) XFAIL("output %d is never written", k);
  if (n == 0) return GPUQ_OK;
  for (int k = 0; k < nouts; k++)
    if (!outs[k]) XFAIL("output %d has no buffer", k);
  for (int c = 0; c < ncols; c++)
    if (!cols[c].data) XFAIL("column %d has no buffer", c);
#undef XFAIL
  a.ninsns = ninsns;
  const int64_t nb = (n + EXPR_TILE - 1) / EXPR_TILE;
  { hipEvent_t _pe = prof_begin(s);
  if (peak <= EXPR_SHALLOW)
    k_expr_eval<EXPR_SHALLOW><<<dim3((uint32_t)nb), EXPR_BLOCK, 0, s>>>(n, a);
  else
    k_expr_eval<GPUQ_EXPR_MAX_DEPTH><<<dim3((uint32_t)nb), EXPR_BLOCK, 0, s>>>(n, a);
  prof_end("project_expr", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* int64 -> float64 cast (AVG = SUM/COUNT evaluation; Average.scala
 * evaluateExpression divides sum by count cast to double) */
__global__ void k_cast_i64_f64(int64_t n, const int64_t* in, double* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (double)in[i];
}

extern "C" int gpuq_cast_i64_f64(void* stream, int64_t n, const int64_t* in,
                                 double* out) {
  k_cast_i64_f64<<<grid1d(n), 256, 0, (hipStream_t)stream>>>(n, in, out);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* RangeExec scan feed (basicPhysicalOperators.scala:630): id = start + i*step */
__global__ void k_range_i64(int64_t n, int64_t start, int64_t step, int64_t* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  /* wraps like Java long arithmetic (unsigned: no signed-overflow UB) */
  for (; i < n; i += stride)
    out[i] = (int64_t)((uint64_t)start + (uint64_t)i * (uint64_t)step);
}

extern "C" int gpuq_range_i64(void* stream, int64_t n, int64_t start,
                              int64_t step, int64_t* out) {
  k_range_i64<<<grid1d(n), 256, 0, (hipStream_t)stream>>>(n, start, step, out);
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ================= WINDOW (segmented scan) ================= */
/*
 * The device side of WindowExec (execution/window/WindowExec.scala; frames as
 * WindowFunctionFrame.scala's UnboundedPrecedingWindowFunctionFrame and
 * UnboundedWindowFunctionFrame evaluate them). The input is already sorted by
 * (partition keys, order keys); nothing here sorts. Partition and peer-group
 * starts are two bitmaps of one bit per row, and every function is a
 * segmented scan under them:
 *
 *  bounds  k_win_bounds: one block per WIN_TILE rows, 8 rows per thread laid
 *          out as in k_pred_mask, so a wave's ballot is one bitmap word.
 *  reduce  k_win_reduce: per tile, the accumulator and non-NULL count since
 *          the tile's last partition start, a has-boundary flag, and the
 *          first / last set bit of both bitmaps.
 *  carry   k_win_carry: one block walks the tile summaries forward,
 *          WIN_CARRY_SPAN at a time with a running carry: the exclusive
 *          segmented scan (f1,a1)+(f2,a2) = (f1|f2, f2 ? a2 : a1 op a2) and a
 *          prefix max of the last-boundary positions. A second block, which
 *          shares nothing with the first, walks them backward for the suffix
 *          min of the first-boundary positions.
 *  apply   k_win_apply: re-reads the tile, scans it seeded with the carry and
 *          writes the ROWS-frame result and its validity bits.
 *  spread  k_win_spread (RANGE / PARTITION frames): out[i] = out[end(i)].
 *  rank / shift read only the bitmaps and the carried positions.
 * Bounded phases, no lookback and no spin-wait (the filter's shape).
 *
 * Row (r, t) of a block is base + r * WIN_BLOCK + t: in round r wave w covers
 * the 64 rows of tile word r * WIN_WAVES + w. The flags of a word-level scan
 * are that word itself, so a lane finds the first lane of its segment with a
 * clz and only the accumulator travels through shuffles; the count of
 * non-NULL rows is a popcount of the validity ballot over the same lanes.
 */
typedef unsigned long long wu64;

#define WIN_BLOCK 256
#define WIN_WAVES (WIN_BLOCK / WAVE)
#define WIN_ITEMS 8
#define WIN_TILE (WIN_BLOCK * WIN_ITEMS)     /* 2048 rows per block */
#define WIN_WORDS (WIN_TILE / WAVE)          /* 32 bitmap words per tile */
#define WIN_CARRY_ITEMS 8
#define WIN_CARRY_SPAN (WIN_BLOCK * WIN_CARRY_ITEMS)  /* tiles per carry step */
#define WIN_MAX_KEYS 8

/* scan operator */
#define WK_NONE 0      /* positions only (ROW_NUMBER, RANK, shift) */
#define WK_ADD_U64 1
#define WK_ADD_F64 2
#define WK_MIN 3       /* on the monotone u64 encodings */
#define WK_MAX 4
/* what a row contributes */
#define WS_RAW 0       /* the column word (SUM) */
#define WS_ENC_I64 1
#define WS_ENC_F64 2
#define WS_VALID 3     /* 1 per non-NULL row: COUNT(col) */
#define WS_ONE 4       /* 1 per row: COUNT(*) */
#define WS_PEER 5      /* the row's peer-start bit: DENSE_RANK */

template <int KIND> DEV wu64 win_ident() { return KIND == WK_MIN ? ~0ULL : 0ULL; }

template <int KIND> DEV wu64 win_op(wu64 a, wu64 b) {
  if (KIND == WK_ADD_F64)
    return (wu64)__double_as_longlong(__longlong_as_double((long long)a) +
                                      __longlong_as_double((long long)b));
  if (KIND == WK_MIN) return a < b ? a : b;
  if (KIND == WK_MAX) return a > b ? a : b;
  return a + b;
}

/* lanes 0..lane */
DEV wu64 win_le_mask(int lane) { return lane == 63 ? ~0ULL : ((2ULL << lane) - 1); }

/* One row's contribution. ok: the row counts as a non-NULL input. A float64
 * SUM addend goes through 0.0 + v, so a -0.0 enters as the +0.0 the running
 * sum would make of it anyway and the result does not depend on where the
 * tile and word edges fall. */
template <int KIND>
DEV wu64 win_elem(int src, const wu64* d, const uint8_t* v, wu64 peer_word,
                  int lane, int64_t i, bool in, bool* ok) {
  if (KIND == WK_NONE) { *ok = false; return 0; }
  if (src == WS_ONE) { *ok = in; return in ? 1ULL : 0ULL; }
  if (src == WS_PEER) { *ok = in; return (peer_word >> lane) & 1; }
  bool valid = in && bit_valid(v, i);
  *ok = valid;
  if (src == WS_VALID) return valid ? 1ULL : 0ULL;
  if (!valid) return win_ident<KIND>();
  wu64 x = d[i];
  if (src == WS_ENC_I64) return encode_i64((int64_t)x);
  if (src == WS_ENC_F64) return encode_f64(__longlong_as_double((long long)x));
  if (KIND == WK_ADD_F64)
    return (wu64)__double_as_longlong(0.0 + __longlong_as_double((long long)x));
  return x;
}

/* inclusive scan over the lanes seg0..lane of a wave (seg0: first lane of the
 * caller's segment, the same in every lane of that segment) */
template <int KIND>
DEV wu64 win_wave_scan(wu64 x, int lane, int seg0) {
  #pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    wu64 y = __shfl_up(x, off);
    if (lane >= off + seg0) x = win_op<KIND>(y, x);
  }
  return x;
}

DEV uint32_t win_wave_max_scan(uint32_t v, int lane) {
  #pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    uint32_t y = __shfl_up(v, off);
    if (lane >= off && y > v) v = y;
  }
  return v;
}

/* v[lane] = min over lanes lane..63 */
DEV uint32_t win_wave_min_rscan(uint32_t v, int lane) {
  #pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    uint32_t y = __shfl_down(v, off);
    if (lane + off < WAVE && y < v) v = y;
  }
  return v;
}

/* Called by one whole wave. tab[w], w < WIN_WORDS: the last set bit of `bits`
 * in the tile's words before w, or prev (the last set bit before the tile)
 * when there is none. Positions ascend, so "last" is a prefix max. */
DEV void win_begin_table(const wu64* bits, int64_t nwords, int64_t tile,
                         uint32_t prev, uint32_t* tab, int lane) {
  int64_t gw = tile * WIN_WORDS + lane;
  wu64 m = (lane < WIN_WORDS && gw < nwords) ? bits[gw] : 0;
  uint32_t v = m ? (uint32_t)(gw * WAVE + 63 - __clzll((long long)m)) : prev;
  v = win_wave_max_scan(v, lane);
  uint32_t e = __shfl_up(v, 1);
  if (lane == 0) e = prev;
  if (lane < WIN_WORDS) tab[lane] = e;
}

/* tab[w]: the first set bit in the tile's words after w, or next (the first
 * set bit after the tile; nrows when there is none). */
DEV void win_end_table(const wu64* bits, int64_t nwords, int64_t tile,
                       uint32_t next, uint32_t* tab, int lane) {
  int64_t gw = tile * WIN_WORDS + lane;
  wu64 m = (lane < WIN_WORDS && gw < nwords) ? bits[gw] : 0;
  uint32_t v = m ? (uint32_t)(gw * WAVE + __ffsll((long long)m) - 1) : next;
  v = win_wave_min_rscan(v, lane);
  uint32_t e = __shfl_down(v, 1);   /* lane 31 reads lane 32, which holds next */
  if (lane < WIN_WORDS) tab[lane] = e;
}

/* last set bit of word m at or before `lane`, as a row position; tab_w when
 * the word has none there */
DEV uint32_t win_begin_of(wu64 m, int lane, int64_t word_base, uint32_t tab_w) {
  wu64 le = m & win_le_mask(lane);
  return le ? (uint32_t)(word_base + 63 - __clzll((long long)le)) : tab_w;
}

/* last row of the group that holds `lane`: the next set bit after it, minus 1 */
DEV uint32_t win_end_of(wu64 m, int lane, int64_t word_base, uint32_t tab_w,
                        int64_t n) {
  wu64 gt = m & ~win_le_mask(lane);
  uint32_t nb = gt ? (uint32_t)(word_base + __ffsll((long long)gt) - 1) : tab_w;
  if (nb > n) nb = (uint32_t)n;   /* a bitmap with bits past nrows reads nothing there */
  return nb - 1;
}

/* validity bits of 64 consecutive rows from their ballot: lanes 0..7 store
 * one byte each; bytes past the bitmap's (nrows + 7) / 8 are not touched */
DEV void win_store_valid(uint8_t* bits, int64_t nbytes, int64_t gw, wu64 m, int lane) {
  if (bits && lane < 8) {
    int64_t b = gw * 8 + lane;
    if (b < nbytes) bits[b] = (uint8_t)(m >> (8 * lane));
  }
}

struct win_keys {
  const wu64* data[WIN_MAX_KEYS];
  const uint8_t* validity[WIN_MAX_KEYS];
  int32_t dtype[WIN_MAX_KEYS];
  int32_t nkeys, npart;
};

/* Each row compares itself with row i-1 in every key column. The neighbour
 * comes from the lane below; lane 0 of a wave loads it (the same line the
 * wave before it streams). Equality is the sort's: both NULL, or both valid
 * with equal encodings (encode_f64: -0.0 == 0.0, one NaN). */
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_bounds(int64_t n, win_keys k, wu64* part, wu64* peer) {
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t base = (int64_t)blockIdx.x * WIN_TILE + threadIdx.x;
  uint32_t pd = 0, od = 0;   /* bit r: row r differs from its predecessor */
  for (int c = 0; c < k.nkeys; c++) {
    const wu64* d = k.data[c];
    const uint8_t* v = k.validity[c];
    const bool f64 = k.dtype[c] == GPUQ_FLOAT64;
    uint32_t diff = 0;
    #pragma unroll
    for (int r = 0; r < WIN_ITEMS; r++) {
      const int64_t i = base + r * WIN_BLOCK;
      const bool in = i < n;
      wu64 cur = in ? d[i] : 0;
      if (f64) cur = encode_f64(__longlong_as_double((long long)cur));
      int cv = in && bit_valid(v, i);
      wu64 prev = __shfl_up(cur, 1);
      int pv = __shfl_up(cv, 1);
      if (lane == 0 && in && i > 0) {
        prev = d[i - 1];
        if (f64) prev = encode_f64(__longlong_as_double((long long)prev));
        pv = bit_valid(v, i - 1);
      }
      bool ne = cv != pv || (cv && cur != prev);
      diff |= (uint32_t)(in && ne) << r;
    }
    if (c < k.npart) pd |= diff; else od |= diff;
  }
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int64_t i = base + r * WIN_BLOCK;
    bool p = i < n && (i == 0 || ((pd >> r) & 1));
    bool q = i < n && (p || ((od >> r) & 1));
    wu64 mp = __ballot(p), mq = __ballot(q);
    int64_t gw = (int64_t)blockIdx.x * WIN_WORDS + r * WIN_WAVES + wave;
    if (lane == 0 && gw < nwords) { part[gw] = mp; peer[gw] = mq; }
  }
}

/* per-tile summaries (reduce) and carries (carry), one entry per tile */
struct win_ws {
  wu64* sum_acc;        /* accumulator since the tile's last partition start */
  wu64* car_acc;        /* accumulator carried INTO the tile */
  uint32_t* sum_cnt;    /* non-NULL rows since the tile's last partition start */
  uint32_t* sum_flag;   /* the tile holds a partition start */
  uint32_t* first_part; /* first / last set bit of the tile, nrows / 0 if none */
  uint32_t* last_part;
  uint32_t* first_peer;
  uint32_t* last_peer;
  uint32_t* car_cnt;
  uint32_t* prev_part;  /* last set bit before the tile */
  uint32_t* prev_peer;
  uint32_t* next_part;  /* first set bit after the tile, nrows if none */
  uint32_t* next_peer;
};

static void win_ws_layout(int64_t n, win_ws* w, char* basep, int64_t* total) {
  int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = basep ? basep + off : nullptr;
    off += (bytes + 255) & ~255LL;
    return p;
  };
  w->sum_acc = (wu64*)take(nt * 8);
  w->car_acc = (wu64*)take(nt * 8);
  uint32_t** u32s[] = {&w->sum_cnt, &w->sum_flag, &w->first_part, &w->last_part,
                       &w->first_peer, &w->last_peer, &w->car_cnt, &w->prev_part,
                       &w->prev_peer, &w->next_part, &w->next_peer};
  for (auto p : u32s) *p = (uint32_t*)take(nt * 4);
  *total = off;
}

extern "C" int64_t gpuq_window_workspace_bytes(int64_t n) {
  if (n < 0) n = 0;
  win_ws w; int64_t total;
  win_ws_layout(n, &w, nullptr, &total);
  return total;
}

/* Wave 0 finds the first / last set bit of both bitmaps in the tile; then
 * (KIND != WK_NONE) every row at or after the last partition start — every
 * row of the tile when it has none — is folded into the tile's accumulator.
 * A missing first bit is stored as nrows and a missing last bit as 0 (row 0
 * starts a partition and a peer group, so 0 is the carry's neutral value). */
template <int KIND>
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_reduce(int64_t n, int src, const wu64* d, const uint8_t* v,
                  const wu64* part, const wu64* peer, win_ws w) {
  __shared__ int s_last;             /* tile-relative, -1: no partition start */
  __shared__ wu64 s_acc[WIN_WAVES];
  __shared__ uint32_t s_cnt[WIN_WAVES];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t tile = blockIdx.x;
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  if (wave == 0) {
    int64_t gw = tile * WIN_WORDS + lane;
    bool have = lane < WIN_WORDS && gw < nwords;
    wu64 mp = have ? part[gw] : 0, mq = have ? peer[gw] : 0;
    wu64 bp = __ballot(mp != 0), bq = __ballot(mq != 0);
    int wlp = bp ? 63 - __clzll((long long)bp) : 0, wfp = bp ? __ffsll((long long)bp) - 1 : 0;
    int wlq = bq ? 63 - __clzll((long long)bq) : 0, wfq = bq ? __ffsll((long long)bq) - 1 : 0;
    wu64 lpw = __shfl(mp, wlp), fpw = __shfl(mp, wfp);
    wu64 lqw = __shfl(mq, wlq), fqw = __shfl(mq, wfq);
    if (lane == 0) {
      const int64_t tb = tile * WIN_TILE;
      int lastrel = bp ? wlp * WAVE + 63 - __clzll((long long)lpw) : -1;
      s_last = lastrel;
      w.sum_flag[tile] = bp != 0;
      w.last_part[tile] = bp ? (uint32_t)(tb + lastrel) : 0u;
      w.first_part[tile] = bp ? (uint32_t)(tb + wfp * WAVE + __ffsll((long long)fpw) - 1)
                              : (uint32_t)n;
      w.last_peer[tile] = bq ? (uint32_t)(tb + wlq * WAVE + 63 - __clzll((long long)lqw)) : 0u;
      w.first_peer[tile] = bq ? (uint32_t)(tb + wfq * WAVE + __ffsll((long long)fqw) - 1)
                              : (uint32_t)n;
    }
  }
  if (KIND == WK_NONE) return;
  /* the rows are loaded before the barrier, so the loads do not wait for
   * wave 0's bitmap words */
  wu64 x[WIN_ITEMS];
  uint32_t okb = 0;
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int64_t gw = tile * WIN_WORDS + r * WIN_WAVES + wave;
    const int64_t i = gw * WAVE + lane;
    wu64 pw = (src == WS_PEER && gw < nwords) ? peer[gw] : 0;
    bool ok;
    x[r] = win_elem<KIND>(src, d, v, pw, lane, i, i < n, &ok);
    okb |= (uint32_t)ok << r;
  }
  __syncthreads();
  const int lastrel = s_last;
  wu64 acc = win_ident<KIND>();
  uint32_t cnt = 0;
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    if ((r * WIN_WAVES + wave) * WAVE + lane >= lastrel) {
      acc = win_op<KIND>(acc, x[r]);
      cnt += (okb >> r) & 1;
    }
  }
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    acc = win_op<KIND>(acc, __shfl_down(acc, off));
    cnt += __shfl_down(cnt, off);
  }
  if (lane == 0) { s_acc[wave] = acc; s_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    #pragma unroll
    for (int k = 1; k < WIN_WAVES; k++) {
      acc = win_op<KIND>(acc, s_acc[k]);
      cnt += s_cnt[k];
    }
    w.sum_acc[tile] = acc;
    w.sum_cnt[tile] = cnt;
  }
}

/* Two blocks that never talk to each other: block 0 walks the tiles forward,
 * block 1 backward. Forward: thread t of a step owns WIN_CARRY_ITEMS
 * consecutive tiles; it folds them, the block scans the 256 thread totals
 * (wave scan with the flag ballot, then the 4 wave totals in order), and the
 * thread walks its tiles again writing the value carried INTO each. `run` is
 * the carry out of the previous step, recomputed identically by every
 * thread. Backward: the same walk from the last tile for the suffix min of
 * the first-boundary positions. ntiles <= 2^21, so at most 1024 steps. */
template <int KIND>
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_carry(int64_t ntiles, uint32_t n, win_ws w) {
  __shared__ wu64 s_acc[WIN_WAVES];
  __shared__ uint32_t s_cnt[WIN_WAVES], s_flag[WIN_WAVES], s_pp[WIN_WAVES], s_pq[WIN_WAVES];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  wu64 run_acc = win_ident<KIND>();
  uint32_t run_cnt = 0, run_pp = 0, run_pq = 0;
  for (int64_t base = 0; blockIdx.x == 0 && base < ntiles; base += WIN_CARRY_SPAN) {
    const int64_t t0 = base + (int64_t)threadIdx.x * WIN_CARRY_ITEMS;
    /* this thread's tiles, loaded back to back (tiles past the end are
     * neutral), then folded: (f, a, c) and the last boundary positions */
    uint32_t tf[WIN_CARRY_ITEMS], tc[WIN_CARRY_ITEMS], tlp[WIN_CARRY_ITEMS],
        tlq[WIN_CARRY_ITEMS];
    wu64 ta[WIN_CARRY_ITEMS];
    #pragma unroll
    for (int k = 0; k < WIN_CARRY_ITEMS; k++) {
      const int64_t t = t0 + k;
      const bool have = t < ntiles;
      tf[k] = (KIND != WK_NONE && have) ? w.sum_flag[t] : 0;
      ta[k] = (KIND != WK_NONE && have) ? w.sum_acc[t] : win_ident<KIND>();
      tc[k] = (KIND != WK_NONE && have) ? w.sum_cnt[t] : 0;
      tlp[k] = have ? w.last_part[t] : 0;
      tlq[k] = have ? w.last_peer[t] : 0;
    }
    uint32_t f = 0, c = 0, pp = 0, pq = 0;
    wu64 a = win_ident<KIND>();
    #pragma unroll
    for (int k = 0; k < WIN_CARRY_ITEMS; k++) {
      if (KIND != WK_NONE) {
        if (tf[k]) { f = 1; a = ta[k]; c = tc[k]; }
        else { a = win_op<KIND>(a, ta[k]); c += tc[k]; }
      }
      pp = tlp[k] > pp ? tlp[k] : pp;
      pq = tlq[k] > pq ? tlq[k] : pq;
    }
    /* inclusive scan across the wave */
    const wu64 fm = __ballot(f != 0);
    const wu64 fle = fm & win_le_mask(lane);
    const int seg0 = fle ? 63 - __clzll((long long)fle) : 0;
    wu64 ia = a;
    uint32_t ic = c;
    if (KIND != WK_NONE) {
      ia = win_wave_scan<KIND>(a, lane, seg0);
      #pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        uint32_t y = __shfl_up(ic, off);
        if (lane >= off + seg0) ic += y;
      }
    }
    const uint32_t ipp = win_wave_max_scan(pp, lane), ipq = win_wave_max_scan(pq, lane);
    if (lane == WAVE - 1) {
      s_acc[wave] = ia; s_cnt[wave] = ic; s_flag[wave] = fm != 0;
      s_pp[wave] = ipp; s_pq[wave] = ipq;
    }
    __syncthreads();
    /* carry into this wave, and (same loop, run to the end) out of the step */
    wu64 wa = run_acc;
    uint32_t wc = run_cnt, wpp = run_pp, wpq = run_pq;
    wu64 in_a = wa;
    uint32_t in_c = wc, in_pp = wpp, in_pq = wpq;
    #pragma unroll
    for (int k = 0; k < WIN_WAVES; k++) {
      if (k == wave) { in_a = wa; in_c = wc; in_pp = wpp; in_pq = wpq; }
      if (KIND != WK_NONE) {
        if (s_flag[k]) { wa = s_acc[k]; wc = s_cnt[k]; }
        else { wa = win_op<KIND>(wa, s_acc[k]); wc += s_cnt[k]; }
      }
      wpp = s_pp[k] > wpp ? s_pp[k] : wpp;
      wpq = s_pq[k] > wpq ? s_pq[k] : wpq;
    }
    run_acc = wa; run_cnt = wc; run_pp = wpp; run_pq = wpq;
    /* exclusive value of this thread: the lane below, under the wave carry */
    wu64 ea = __shfl_up(ia, 1);
    uint32_t ec = __shfl_up(ic, 1);
    uint32_t epp = __shfl_up(ipp, 1), epq = __shfl_up(ipq, 1);
    const bool flag_below = (fm & (win_le_mask(lane) >> 1)) != 0;
    if (lane == 0) { ea = in_a; ec = in_c; epp = in_pp; epq = in_pq; }
    else {
      if (KIND != WK_NONE && !flag_below) { ea = win_op<KIND>(in_a, ea); ec += in_c; }
      epp = in_pp > epp ? in_pp : epp;
      epq = in_pq > epq ? in_pq : epq;
    }
    #pragma unroll
    for (int k = 0; k < WIN_CARRY_ITEMS; k++) {
      const int64_t t = t0 + k;
      if (t < ntiles) {
        w.prev_part[t] = epp;
        w.prev_peer[t] = epq;
        epp = tlp[k] > epp ? tlp[k] : epp;
        epq = tlq[k] > epq ? tlq[k] : epq;
        if (KIND != WK_NONE) {
          w.car_acc[t] = ea;
          w.car_cnt[t] = ec;
          if (tf[k]) { ea = ta[k]; ec = tc[k]; }
          else { ea = win_op<KIND>(ea, ta[k]); ec += tc[k]; }
        }
      }
    }
    __syncthreads();
  }
  /* suffix min of the first-boundary positions: tile u counts from the end */
  uint32_t run_np = n, run_nq = n;
  for (int64_t base = 0; blockIdx.x == 1 && base < ntiles; base += WIN_CARRY_SPAN) {
    const int64_t u0 = base + (int64_t)threadIdx.x * WIN_CARRY_ITEMS;
    uint32_t tfp[WIN_CARRY_ITEMS], tfq[WIN_CARRY_ITEMS];
    #pragma unroll
    for (int k = 0; k < WIN_CARRY_ITEMS; k++) {
      const int64_t u = u0 + k;
      tfp[k] = u < ntiles ? w.first_part[ntiles - 1 - u] : n;
      tfq[k] = u < ntiles ? w.first_peer[ntiles - 1 - u] : n;
    }
    uint32_t np = n, nq = n;
    #pragma unroll
    for (int k = 0; k < WIN_CARRY_ITEMS; k++) {
      np = tfp[k] < np ? tfp[k] : np;
      nq = tfq[k] < nq ? tfq[k] : nq;
    }
    /* prefix min in u order == suffix min in tile order */
    uint32_t inp = np, inq = nq;
    #pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      uint32_t y = __shfl_up(inp, off), z = __shfl_up(inq, off);
      if (lane >= off) { inp = y < inp ? y : inp; inq = z < inq ? z : inq; }
    }
    if (lane == WAVE - 1) { s_pp[wave] = inp; s_pq[wave] = inq; }
    __syncthreads();
    uint32_t wnp = run_np, wnq = run_nq, in_np = run_np, in_nq = run_nq;
    #pragma unroll
    for (int k = 0; k < WIN_WAVES; k++) {
      if (k == wave) { in_np = wnp; in_nq = wnq; }
      wnp = s_pp[k] < wnp ? s_pp[k] : wnp;
      wnq = s_pq[k] < wnq ? s_pq[k] : wnq;
    }
    run_np = wnp; run_nq = wnq;
    uint32_t enp = __shfl_up(inp, 1), enq = __shfl_up(inq, 1);
    if (lane == 0) { enp = in_np; enq = in_nq; }
    else { enp = in_np < enp ? in_np : enp; enq = in_nq < enq ? in_nq : enq; }
    #pragma unroll
    for (int k = 0; k < WIN_CARRY_ITEMS; k++) {
      const int64_t u = u0 + k;
      if (u < ntiles) {
        const int64_t t = ntiles - 1 - u;
        w.next_part[t] = enp;
        w.next_peer[t] = enq;
        enp = tfp[k] < enp ? tfp[k] : enp;
        enq = tfq[k] < enq ? tfq[k] : enq;
      }
    }
    __syncthreads();
  }
}

/* The ROWS-frame result of every row of the tile. Word scans in registers,
 * their 32 totals scanned by wave 0 under the tile's carry, then each row
 * whose word has no partition start at or before it takes its word's carry.
 * dec: 0 raw word, 1 decode_i64, 2 decode_f64. A row with no non-NULL value
 * in its frame is NULL and holds 0, unless never_null (COUNT, DENSE_RANK). */
template <int KIND>
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_apply(int64_t n, int src, const wu64* d, const uint8_t* v,
                 const wu64* part, const wu64* peer, win_ws w, int dec,
                 int never_null, wu64* out, uint8_t* out_valid, int64_t nbytes) {
  __shared__ wu64 s_acc[WIN_WORDS], s_xacc[WIN_WORDS];
  __shared__ uint32_t s_cnt[WIN_WORDS], s_xcnt[WIN_WORDS], s_flag[WIN_WORDS];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t tile = blockIdx.x;
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  wu64 x[WIN_ITEMS];
  uint32_t c[WIN_ITEMS];
  uint32_t started = 0;   /* bit r: a partition starts at or before this lane in word r */
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int wd = r * WIN_WAVES + wave;
    const int64_t gw = tile * WIN_WORDS + wd;
    const int64_t i = gw * WAVE + lane;
    const wu64 m = gw < nwords ? part[gw] : 0;
    const wu64 pw = (src == WS_PEER && gw < nwords) ? peer[gw] : 0;
    bool ok;
    wu64 e = win_elem<KIND>(src, d, v, pw, lane, i, i < n, &ok);
    const wu64 vm = __ballot(ok);
    const wu64 le = win_le_mask(lane);
    const wu64 mle = m & le;
    const int seg0 = mle ? 63 - __clzll((long long)mle) : 0;
    x[r] = win_wave_scan<KIND>(e, lane, seg0);
    c[r] = (uint32_t)__popcll(vm & le & ~((1ULL << seg0) - 1));
    started |= (uint32_t)(mle != 0) << r;
    if (lane == WAVE - 1) { s_acc[wd] = x[r]; s_cnt[wd] = c[r]; s_flag[wd] = m != 0; }
  }
  __syncthreads();
  if (wave == 0) {
    const wu64 tc_acc = w.car_acc[tile];
    const uint32_t tc_cnt = w.car_cnt[tile];
    wu64 a = lane < WIN_WORDS ? s_acc[lane] : win_ident<KIND>();
    uint32_t cn = lane < WIN_WORDS ? s_cnt[lane] : 0;
    const wu64 fm = __ballot(lane < WIN_WORDS && s_flag[lane] != 0);
    const wu64 fle = fm & win_le_mask(lane);
    const int seg0 = fle ? 63 - __clzll((long long)fle) : 0;
    a = win_wave_scan<KIND>(a, lane, seg0);
    #pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      uint32_t y = __shfl_up(cn, off);
      if (lane >= off + seg0) cn += y;
    }
    if (!fle) { a = win_op<KIND>(tc_acc, a); cn += tc_cnt; }
    /* the value carried into word lane + 1 */
    if (lane < WIN_WORDS - 1) { s_xacc[lane + 1] = a; s_xcnt[lane + 1] = cn; }
    if (lane == 0) { s_xacc[0] = tc_acc; s_xcnt[0] = tc_cnt; }
  }
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int wd = r * WIN_WAVES + wave;
    const int64_t gw = tile * WIN_WORDS + wd;
    const int64_t i = gw * WAVE + lane;
    wu64 a = x[r];
    uint32_t cn = c[r];
    if (!((started >> r) & 1)) { a = win_op<KIND>(s_xacc[wd], a); cn += s_xcnt[wd]; }
    const bool valid = i < n && (never_null || cn > 0);
    if (i < n) {
      wu64 o = 0;
      if (valid)
        o = dec == 1 ? (wu64)decode_i64(a)
          : dec == 2 ? (wu64)__double_as_longlong(decode_f64(a)) : a;
      out[i] = o;
    }
    win_store_valid(out_valid, nbytes, gw, __ballot(valid), lane);
  }
}

/* out[i] = out[end(i)], end(i) the last row of i's group under `bits` (peer
 * starts for RANGE, partition starts for PARTITION), and the same for the
 * validity bit. In place: end(end(i)) == end(i), so a row that others read is
 * rewritten with the value and the bit it already holds. */
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_spread(int64_t n, const wu64* bits, const uint32_t* next,
                  wu64* out, uint8_t* out_valid, int64_t nbytes) {
  __shared__ uint32_t s_end[WIN_WORDS];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t tile = blockIdx.x;
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  if (wave == 0) win_end_table(bits, nwords, tile, next[tile], s_end, lane);
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int wd = r * WIN_WAVES + wave;
    const int64_t gw = tile * WIN_WORDS + wd;
    const int64_t i = gw * WAVE + lane;
    bool valid = false;
    if (i < n) {
      const uint32_t e = win_end_of(bits[gw], lane, gw * WAVE, s_end[wd], n);
      valid = bit_valid(out_valid, e);
      out[i] = out[e];
    }
    win_store_valid(out_valid, nbytes, gw, __ballot(valid), lane);
  }
}

/* ROW_NUMBER = i - part_begin(i) + 1, RANK = peer_begin(i) - part_begin(i) + 1 */
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_rank(int64_t n, int op, const wu64* part, const wu64* peer,
                const uint32_t* prev_part, const uint32_t* prev_peer, int64_t* out,
                uint8_t* out_valid, int64_t nbytes) {
  __shared__ uint32_t s_pb[WIN_WORDS], s_qb[WIN_WORDS];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t tile = blockIdx.x;
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  if (wave == 0) win_begin_table(part, nwords, tile, prev_part[tile], s_pb, lane);
  if (wave == 1) win_begin_table(peer, nwords, tile, prev_peer[tile], s_qb, lane);
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int wd = r * WIN_WAVES + wave;
    const int64_t gw = tile * WIN_WORDS + wd;
    const int64_t i = gw * WAVE + lane;
    if (i < n) {
      const int64_t pb = win_begin_of(part[gw], lane, gw * WAVE, s_pb[wd]);
      const int64_t top = op == GPUQ_WIN_RANK
          ? (int64_t)win_begin_of(peer[gw], lane, gw * WAVE, s_qb[wd]) : i;
      out[i] = top - pb + 1;
    }
    win_store_valid(out_valid, nbytes, gw, __ballot(i < n), lane);
  }
}

/* out[i] = val[i + offset] when that row lies in i's partition */
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_shift(int64_t n, const wu64* d, const uint8_t* v, int64_t offset,
                 int has_default, wu64 dflt, const wu64* part,
                 const uint32_t* prev_part, const uint32_t* next_part,
                 wu64* out, uint8_t* out_valid, int64_t nbytes) {
  __shared__ uint32_t s_pb[WIN_WORDS], s_pe[WIN_WORDS];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t tile = blockIdx.x;
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  if (wave == 0) win_begin_table(part, nwords, tile, prev_part[tile], s_pb, lane);
  if (wave == 1) win_end_table(part, nwords, tile, next_part[tile], s_pe, lane);
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int wd = r * WIN_WAVES + wave;
    const int64_t gw = tile * WIN_WORDS + wd;
    const int64_t i = gw * WAVE + lane;
    bool valid = false;
    if (i < n) {
      const wu64 m = part[gw];
      const int64_t j = i + offset;
      const bool inpart = offset < 0
          ? j >= (int64_t)win_begin_of(m, lane, gw * WAVE, s_pb[wd])
          : j <= (int64_t)win_end_of(m, lane, gw * WAVE, s_pe[wd], n);
      wu64 x = 0;
      if (inpart) {
        valid = bit_valid(v, j);
        if (valid) x = d[j];
      } else if (has_default) {
        valid = true;
        x = dflt;
      }
      out[i] = x;
    }
    win_store_valid(out_valid, nbytes, gw, __ballot(valid), lane);
  }
}

/* ---- sliding ROWS frames (SlidingWindowFunctionFrame) ----
 * Row i of the partition [pb, pe] aggregates the rows first..last, first =
 * max(pb, i + lo), last = min(pe, i + hi); the frame is empty when first >
 * last. Spark re-adds the frame's rows in row order for every output row, and
 * so does k_win_slide: a difference of prefix sums would cancel, turn inf -
 * inf into NaN and let one NaN poison the rest of its partition.
 *
 * One block per WIN_TILE rows in the row layout of the scans. The block
 * stages the rows [tile_base + lo, tile_base + WIN_TILE - 1 + hi] that lie in
 * [0, nrows) once into LDS, element e = row - (tile_base + lo): s_val[e] is
 * the raw word (SUM, FIRST / LAST) or the encode_* word (MIN / MAX), and the
 * operator's identity for a NULL row or a row outside the input, so the loop
 * of a row folds s_val[first..last] without looking at validity (a float64
 * accumulator that starts at +0.0 never becomes -0.0, so adding the +0.0 of a
 * NULL row changes no bit). Validity is staged as one ballot word per 64
 * elements plus the exclusive prefix of their popcounts: the non-NULL count
 * of first..last is two rank lookups, and it alone decides NULL-ness. COUNT
 * and FIRST / LAST need no loop. The 64 lanes of a wave own consecutive rows
 * and their loops start at consecutive elements (clipped lanes of one
 * partition share an address): 8-byte reads of one bank row per half wave.
 * LDS: (WIN_TILE + WIN_SLIDE_MAX_SPAN) * 8 bytes = 32 KiB of values and
 * about 1 KiB of validity words, counts, partition words and tables. */
#define WIN_SLIDE_MAX_SPAN GPUQ_WIN_SLIDE_MAX_SPAN
#define WIN_STAGE (WIN_TILE + WIN_SLIDE_MAX_SPAN)
#define WIN_STAGE_WORDS (WIN_STAGE / WAVE)

#define SK_COUNT 0
#define SK_SUM_U64 1
#define SK_SUM_F64 2
#define SK_MIN 3
#define SK_MAX 4
#define SK_FIRST 5
#define SK_LAST 6

/* non-NULL staged elements before element q, q <= WIN_STAGE */
DEV uint32_t win_stage_rank(const wu64* vw, const uint32_t* vc, int q) {
  return vc[q >> 6] + (uint32_t)__popcll(vw[q >> 6] & ((1ULL << (q & 63)) - 1));
}

template <int KIND>
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_slide(int64_t n, int f64, const wu64* d, const uint8_t* v,
                 int64_t lo, int64_t hi, const wu64* part,
                 const uint32_t* prev_part, const uint32_t* next_part,
                 wu64* out, uint8_t* out_valid, int64_t nbytes) {
  __shared__ wu64 s_val[KIND == SK_COUNT ? 1 : WIN_STAGE];
  __shared__ wu64 s_vw[WIN_STAGE_WORDS + 1];
  __shared__ uint32_t s_vc[WIN_STAGE_WORDS + 1];
  __shared__ uint32_t s_pb[WIN_WORDS], s_pe[WIN_WORDS];
  __shared__ wu64 s_pw[WIN_WORDS];                     /* the tile's partition words */
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t tile = blockIdx.x;
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  const int64_t sbase = tile * WIN_TILE + lo;          /* row of element 0 */
  const int ne = WIN_TILE + (int)(hi - lo);            /* staged elements */
  const int rounds = (ne + WIN_BLOCK - 1) / WIN_BLOCK; /* <= 16 */
  const wu64 ident = KIND == SK_MIN ? ~0ULL : 0ULL;
  if (wave == 0) win_begin_table(part, nwords, tile, prev_part[tile], s_pb, lane);
  if (wave == 1) win_end_table(part, nwords, tile, next_part[tile], s_pe, lane);
  if (wave == 2 && lane < WIN_WORDS) {
    const int64_t gw = tile * WIN_WORDS + lane;
    s_pw[lane] = gw < nwords ? part[gw] : 0;
  }
  for (int k = 0; k < rounds; k++) {
    const int e = k * WIN_BLOCK + threadIdx.x;
    const int64_t row = sbase + e;
    const bool ok = e < ne && row >= 0 && row < n && (!d || bit_valid(v, row));
    if (KIND != SK_COUNT) {
      wu64 x = ident;
      if (ok) {
        x = d[row];
        if (KIND == SK_MIN || KIND == SK_MAX)
          x = f64 ? encode_f64(__longlong_as_double((long long)x))
                  : encode_i64((int64_t)x);
      }
      s_val[e] = x;
    }
    const wu64 m = __ballot(ok);
    if (lane == 0) s_vw[k * WIN_WAVES + wave] = m;
  }
  __syncthreads();
  if (wave == 0) {
    /* words past the staged rounds read as empty; s_vc[w] = non-NULL
     * elements in the words before w */
    const wu64 m = lane < rounds * WIN_WAVES ? s_vw[lane] : 0;
    uint32_t c = (uint32_t)__popcll(m);
    #pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      uint32_t y = __shfl_up(c, off);
      if (lane >= off) c += y;
    }
    s_vw[lane] = m;
    s_vc[lane + 1] = c;
    if (lane == 0) { s_vc[0] = 0; s_vw[WIN_STAGE_WORDS] = 0; }
  }
  __syncthreads();
  #pragma unroll 2
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int wd = r * WIN_WAVES + wave;
    const int64_t gw = tile * WIN_WORDS + wd;
    const int64_t i = gw * WAVE + lane;
    bool valid = false;
    if (i < n) {
      const wu64 m = s_pw[wd];
      const int64_t pb = win_begin_of(m, lane, gw * WAVE, s_pb[wd]);
      const int64_t pe = win_end_of(m, lane, gw * WAVE, s_pe[wd], n);
      const int64_t first = i + lo > pb ? i + lo : pb;
      const int64_t last = i + hi < pe ? i + hi : pe;
      wu64 o = 0;
      valid = KIND == SK_COUNT;
      if (first <= last) {
        /* 0 <= a <= b < ne: first >= tile_base + lo, last <= i + hi */
        const int a = (int)(first - sbase), b = (int)(last - sbase);
        if (KIND == SK_FIRST || KIND == SK_LAST) {
          const int p = KIND == SK_FIRST ? a : b;
          valid = (s_vw[p >> 6] >> (p & 63)) & 1;
          o = s_val[p];
        } else {
          const uint32_t cnt = win_stage_rank(s_vw, s_vc, b + 1) -
                               win_stage_rank(s_vw, s_vc, a);
          if (KIND == SK_COUNT) {
            o = cnt;
          } else if (cnt > 0) {
            valid = true;
            if (KIND == SK_SUM_F64) {
              double acc = 0.0;
              #pragma unroll 4
              for (int p = a; p <= b; p++)
                acc += __longlong_as_double((long long)s_val[p]);
              o = (wu64)__double_as_longlong(acc);
            } else {
              wu64 acc = ident;
              #pragma unroll 4
              for (int p = a; p <= b; p++) {
                const wu64 x = s_val[p];
                acc = KIND == SK_MIN ? (x < acc ? x : acc)
                    : KIND == SK_MAX ? (x > acc ? x : acc) : acc + x;
              }
              o = KIND == SK_SUM_U64 ? acc
                : f64 ? (wu64)__double_as_longlong(decode_f64(acc))
                      : (wu64)decode_i64(acc);
            }
          }
        }
      }
      out[i] = o;
    }
    win_store_valid(out_valid, nbytes, gw, __ballot(valid), lane);
  }
}

/* Frames that start at UNBOUNDED PRECEDING and end hi rows from the row (hi
 * already clamped to [-nrows, nrows]; nrows stands for UNBOUNDED FOLLOWING):
 * the frame of row i is the ROWS-scan frame of row j = min(i + hi, pe), and
 * it is empty when i + hi < pb. mode 0: out[i] = src[j] with src's validity
 * (the scan's result in the workspace); 1: FIRST_VALUE, src[pb]; 2:
 * LAST_VALUE, src[j] (src the value column). An empty frame gives 0, NULL
 * unless never_null. NULL rows hold 0. */
__global__ __launch_bounds__(WIN_BLOCK)
void k_win_pick(int64_t n, int mode, int64_t hi, const wu64* src,
                const uint8_t* src_valid, int never_null, const wu64* part,
                const uint32_t* prev_part, const uint32_t* next_part,
                wu64* out, uint8_t* out_valid, int64_t nbytes) {
  __shared__ uint32_t s_pb[WIN_WORDS], s_pe[WIN_WORDS];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int64_t tile = blockIdx.x;
  const int64_t nwords = (n + WAVE - 1) / WAVE;
  if (wave == 0) win_begin_table(part, nwords, tile, prev_part[tile], s_pb, lane);
  if (wave == 1) win_end_table(part, nwords, tile, next_part[tile], s_pe, lane);
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < WIN_ITEMS; r++) {
    const int wd = r * WIN_WAVES + wave;
    const int64_t gw = tile * WIN_WORDS + wd;
    const int64_t i = gw * WAVE + lane;
    bool valid = false;
    if (i < n) {
      const wu64 m = part[gw];
      const int64_t pb = win_begin_of(m, lane, gw * WAVE, s_pb[wd]);
      const int64_t pe = win_end_of(m, lane, gw * WAVE, s_pe[wd], n);
      const int64_t j = i + hi < pe ? i + hi : pe;
      wu64 o = 0;
      valid = never_null != 0;
      if (j >= pb) {
        const int64_t p = mode == 1 ? pb : j;
        valid = never_null || bit_valid(src_valid, p);
        if (valid) o = src[p];
      }
      out[i] = o;
    }
    win_store_valid(out_valid, nbytes, gw, __ballot(valid), lane);
  }
}

extern "C" int gpuq_window_boundaries(void* stream, int64_t n, const gpuq_col* keys,
                                      int32_t nkeys, int32_t npart,
                                      uint64_t* out_part_start,
                                      uint64_t* out_peer_start) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || n > 0xFFFFFFFFLL)
    FAIL(GPUQ_ERR_INVALID, "window_boundaries: nrows %lld out of range", (long long)n);
  if (nkeys < 0 || nkeys > WIN_MAX_KEYS)
    FAIL(GPUQ_ERR_INVALID, "window_boundaries: %d keys, need 0..%d", nkeys, WIN_MAX_KEYS);
  if (npart < 0 || npart > nkeys)
    FAIL(GPUQ_ERR_INVALID, "window_boundaries: %d partition keys of %d keys", npart, nkeys);
  win_keys k;
  memset(&k, 0, sizeof(k));
  for (int c = 0; c < nkeys; c++) {
    if (keys[c].dtype != GPUQ_INT64 && keys[c].dtype != GPUQ_FLOAT64)
      FAIL(GPUQ_ERR_INVALID, "window_boundaries: key %d has unsupported dtype %d", c, keys[c].dtype);
    k.data[c] = (const wu64*)keys[c].data;
    k.validity[c] = keys[c].validity;
    k.dtype[c] = keys[c].dtype;
  }
  k.nkeys = nkeys; k.npart = npart;
  if (n == 0) return GPUQ_OK;
  const int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  { hipEvent_t _pe = prof_begin(s);
  k_win_bounds<<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
      n, k, (wu64*)out_part_start, (wu64*)out_peer_start);
  prof_end("win_bounds", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* reduce + carry for one scan operator */
template <int KIND>
static void win_reduce_carry(hipStream_t s, int64_t n, int src, gpuq_col val,
                             const uint64_t* part, const uint64_t* peer, win_ws& w) {
  const int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  { hipEvent_t _pe = prof_begin(s);
  k_win_reduce<KIND><<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
      n, src, (const wu64*)val.data, val.validity, (const wu64*)part,
      (const wu64*)peer, w);
  prof_end("win_reduce", s, _pe); }
  { hipEvent_t _pe = prof_begin(s);
  k_win_carry<KIND><<<2, WIN_BLOCK, 0, s>>>(nt, (uint32_t)n, w);
  prof_end("win_carry", s, _pe); }
}

template <int KIND>
static void win_scan_rows(hipStream_t s, int64_t n, int src, gpuq_col val,
                          const uint64_t* part, const uint64_t* peer, win_ws& w,
                          int dec, int never_null, void* out, uint8_t* out_valid) {
  const int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  win_reduce_carry<KIND>(s, n, src, val, part, peer, w);
  { hipEvent_t _pe = prof_begin(s);
  k_win_apply<KIND><<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
      n, src, (const wu64*)val.data, val.validity, (const wu64*)part,
      (const wu64*)peer, w, dec, never_null, (wu64*)out, out_valid, (n + 7) / 8);
  prof_end("win_apply", s, _pe); }
}

extern "C" int gpuq_window_scan(void* stream, int64_t n, int32_t op, int32_t frame,
                                gpuq_col val, const uint64_t* part_start,
                                const uint64_t* peer_start, void* out,
                                uint8_t* out_validity_bits,
                                void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || n > 0xFFFFFFFFLL)
    FAIL(GPUQ_ERR_INVALID, "window_scan: nrows %lld out of range", (long long)n);
  if (op < GPUQ_WIN_ROW_NUMBER || op > GPUQ_WIN_MAX)
    FAIL(GPUQ_ERR_INVALID, "window_scan: bad op %d", op);
  if (frame < GPUQ_FRAME_ROWS || frame > GPUQ_FRAME_PARTITION)
    FAIL(GPUQ_ERR_INVALID, "window_scan: bad frame %d", frame);
  const bool rank_op = op <= GPUQ_WIN_DENSE_RANK;
  if (rank_op && frame != GPUQ_FRAME_ROWS)
    FAIL(GPUQ_ERR_INVALID, "window_scan: rank op %d takes the ROWS frame only", op);
  const bool reads_val = !rank_op && (op != GPUQ_WIN_COUNT || val.data);
  /* an empty column's pointer may be NULL */
  if (n > 0 && !rank_op && op != GPUQ_WIN_COUNT && !val.data)
    FAIL(GPUQ_ERR_INVALID, "window_scan: op %d needs a value column", op);
  if (reads_val && val.dtype != GPUQ_INT64 && val.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "window_scan: unsupported dtype %d", val.dtype);
  const bool never_null = rank_op || op == GPUQ_WIN_COUNT;
  if (!never_null && val.validity && !out_validity_bits)
    FAIL(GPUQ_ERR_INVALID, "window_scan: a nullable value column needs an output bitmap");
  win_ws w; int64_t need;
  win_ws_layout(n, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "window_scan: workspace %lld < %lld",
         (long long)workspace_bytes, (long long)need);
  if (n == 0) return GPUQ_OK;
  const int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  const bool f64 = val.dtype == GPUQ_FLOAT64;
  if (!reads_val) val.validity = nullptr;
  switch (op) {
    case GPUQ_WIN_ROW_NUMBER:
    case GPUQ_WIN_RANK:
      win_reduce_carry<WK_NONE>(s, n, WS_ONE, val, part_start, peer_start, w);
      { hipEvent_t _pe = prof_begin(s);
      k_win_rank<<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
          n, op, (const wu64*)part_start, (const wu64*)peer_start,
          w.prev_part, w.prev_peer, (int64_t*)out, out_validity_bits, (n + 7) / 8);
      prof_end("win_apply", s, _pe); }
      break;
    case GPUQ_WIN_DENSE_RANK:
      win_scan_rows<WK_ADD_U64>(s, n, WS_PEER, val, part_start, peer_start, w, 0, 1,
                                out, out_validity_bits);
      break;
    case GPUQ_WIN_COUNT:
      win_scan_rows<WK_ADD_U64>(s, n, val.data ? WS_VALID : WS_ONE, val, part_start,
                                peer_start, w, 0, 1, out, out_validity_bits);
      break;
    case GPUQ_WIN_SUM:
      if (f64) win_scan_rows<WK_ADD_F64>(s, n, WS_RAW, val, part_start, peer_start, w,
                                         0, 0, out, out_validity_bits);
      else win_scan_rows<WK_ADD_U64>(s, n, WS_RAW, val, part_start, peer_start, w,
                                     0, 0, out, out_validity_bits);
      break;
    case GPUQ_WIN_MIN:
      win_scan_rows<WK_MIN>(s, n, f64 ? WS_ENC_F64 : WS_ENC_I64, val, part_start,
                            peer_start, w, f64 ? 2 : 1, 0, out, out_validity_bits);
      break;
    default:
      win_scan_rows<WK_MAX>(s, n, f64 ? WS_ENC_F64 : WS_ENC_I64, val, part_start,
                            peer_start, w, f64 ? 2 : 1, 0, out, out_validity_bits);
      break;
  }
  HIP_TRY(hipGetLastError());
  if (frame != GPUQ_FRAME_ROWS) {
    const bool range = frame == GPUQ_FRAME_RANGE;
    { hipEvent_t _pe = prof_begin(s);
    k_win_spread<<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
        n, (const wu64*)(range ? peer_start : part_start),
        range ? w.next_peer : w.next_part, (wu64*)out, out_validity_bits, (n + 7) / 8);
    prof_end("win_spread", s, _pe); }
    HIP_TRY(hipGetLastError());
  }
  return GPUQ_OK;
}

extern "C" int gpuq_window_shift(void* stream, int64_t n, gpuq_col val, int64_t offset,
                                 int32_t has_default, double lit_f64, int64_t lit_i64,
                                 const uint64_t* part_start, void* out,
                                 uint8_t* out_validity_bits,
                                 void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || n > 0xFFFFFFFFLL)
    FAIL(GPUQ_ERR_INVALID, "window_shift: nrows %lld out of range", (long long)n);
  if (val.dtype != GPUQ_INT64 && val.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "window_shift: unsupported dtype %d", val.dtype);
  win_ws w; int64_t need;
  win_ws_layout(n, &w, (char*)workspace, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "window_shift: workspace %lld < %lld",
         (long long)workspace_bytes, (long long)need);
  if (n == 0) return GPUQ_OK;
  if (!val.data) FAIL(GPUQ_ERR_INVALID, "window_shift: needs a value column");
  if (!out_validity_bits) FAIL(GPUQ_ERR_INVALID, "window_shift: needs an output bitmap");
  /* an offset past either end of the input is past every partition */
  if (offset > n) offset = n;
  if (offset < -n) offset = -n;
  wu64 dflt;
  if (val.dtype == GPUQ_FLOAT64) memcpy(&dflt, &lit_f64, 8);
  else memcpy(&dflt, &lit_i64, 8);
  const int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  /* the peer bitmap is not needed: the partition bitmap stands in for it */
  win_reduce_carry<WK_NONE>(s, n, WS_ONE, val, part_start, part_start, w);
  { hipEvent_t _pe = prof_begin(s);
  k_win_shift<<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
      n, (const wu64*)val.data, val.validity, offset, has_default != 0, dflt,
      (const wu64*)part_start, w.prev_part, w.next_part, (wu64*)out,
      out_validity_bits, (n + 7) / 8);
  prof_end("win_shift", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}

/* ---- sliding frames: host side ---- */

/* NULL when (lo, hi) is a frame gpuq_window_slide runs, else what is wrong */
static const char* win_slide_frame_error(int64_t lo, int64_t hi) {
  const bool lo_unb = lo == GPUQ_WIN_UNBOUNDED_PRECEDING;
  const bool hi_unb = hi == GPUQ_WIN_UNBOUNDED_FOLLOWING;
  if (!lo_unb && (lo < INT32_MIN || lo > INT32_MAX)) return "lo does not fit int32";
  if (!hi_unb && (hi < INT32_MIN || hi > INT32_MAX)) return "hi does not fit int32";
  if (!lo_unb && hi_unb)
    return "a finite lo with UNBOUNDED FOLLOWING is not supported";
  if (!lo_unb && lo > hi) return "lo > hi";
  if (!lo_unb && hi - lo > GPUQ_WIN_SLIDE_MAX_SPAN) return "span hi - lo over the cap";
  return nullptr;
}

/* the scan's workspace first; frames from UNBOUNDED PRECEDING add the scan's
 * result: nrows words and a bitmap */
static void win_slide_ws_layout(int64_t n, int64_t lo, win_ws* w, char* basep,
                                wu64** tmp, uint8_t** tmp_valid, int64_t* total) {
  int64_t off;
  win_ws_layout(n, w, basep, &off);
  *tmp = nullptr; *tmp_valid = nullptr;
  if (lo == GPUQ_WIN_UNBOUNDED_PRECEDING) {
    *tmp = (wu64*)(basep ? basep + off : nullptr);
    off += (n * 8 + 255) & ~255LL;
    *tmp_valid = (uint8_t*)(basep ? basep + off : nullptr);
    off += ((n + 7) / 8 + 255) & ~255LL;
  }
  *total = off;
}

extern "C" int64_t gpuq_window_slide_workspace_bytes(int64_t n, int64_t lo, int64_t hi) {
  if (n < 0 || n > 0xFFFFFFFFLL || win_slide_frame_error(lo, hi)) return 0;
  win_ws w; wu64* tmp; uint8_t* tv; int64_t total;
  win_slide_ws_layout(n, lo, &w, nullptr, &tmp, &tv, &total);
  return total;
}

template <int KIND>
static void win_slide_launch(hipStream_t s, int64_t n, int f64, gpuq_col val,
                             int64_t lo, int64_t hi, const uint64_t* part,
                             win_ws& w, void* out, uint8_t* out_valid) {
  const int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  hipEvent_t _pe = prof_begin(s);
  k_win_slide<KIND><<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
      n, f64, (const wu64*)val.data, val.validity, lo, hi, (const wu64*)part,
      w.prev_part, w.next_part, (wu64*)out, out_valid, (n + 7) / 8);
  prof_end("win_slide", s, _pe);
}

extern "C" int gpuq_window_slide(void* stream, int64_t n, int32_t op, gpuq_col val,
                                 int64_t lo, int64_t hi, const uint64_t* part_start,
                                 void* out, uint8_t* out_validity_bits,
                                 void* workspace, int64_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || n > 0xFFFFFFFFLL)
    FAIL(GPUQ_ERR_INVALID, "window_slide: nrows %lld out of range", (long long)n);
  if (op < GPUQ_WIN_COUNT || op > GPUQ_WIN_LAST_VALUE)
    FAIL(GPUQ_ERR_INVALID, "window_slide: bad op %d", op);
  const bool reads_val = op != GPUQ_WIN_COUNT || val.data;
  if (reads_val && val.dtype != GPUQ_INT64 && val.dtype != GPUQ_FLOAT64)
    FAIL(GPUQ_ERR_INVALID, "window_slide: unsupported dtype %d", val.dtype);
  /* an empty column's pointer may be NULL */
  if (n > 0 && op != GPUQ_WIN_COUNT && !val.data)
    FAIL(GPUQ_ERR_INVALID, "window_slide: op %d needs a value column", op);
  if (const char* why = win_slide_frame_error(lo, hi))
    FAIL(GPUQ_ERR_INVALID, "window_slide: bad frame (%lld, %lld): %s",
         (long long)lo, (long long)hi, why);
  const bool lo_unb = lo == GPUQ_WIN_UNBOUNDED_PRECEDING;
  const bool pick_val = op >= GPUQ_WIN_FIRST_VALUE;
  const bool can_be_empty = (!lo_unb && lo > 0) || hi < 0;
  /* an empty bitmap's pointer may be NULL too */
  if (n > 0 && !out_validity_bits &&
      (pick_val || (op != GPUQ_WIN_COUNT && (val.validity || can_be_empty))))
    FAIL(GPUQ_ERR_INVALID, "window_slide: op %d over this column and frame "
         "needs an output bitmap", op);
  win_ws w; wu64* tmp; uint8_t* tmp_valid; int64_t need;
  win_slide_ws_layout(n, lo, &w, (char*)workspace, &tmp, &tmp_valid, &need);
  if (workspace_bytes < need)
    FAIL(GPUQ_ERR_INVALID, "window_slide: workspace %lld < %lld",
         (long long)workspace_bytes, (long long)need);
  if (n == 0) return GPUQ_OK;
  const int64_t nt = (n + WIN_TILE - 1) / WIN_TILE;
  const int f64 = val.dtype == GPUQ_FLOAT64;
  if (!reads_val) val.validity = nullptr;
  if (!lo_unb) {
    /* positions only; the partition bitmap stands in for the peer bitmap */
    win_reduce_carry<WK_NONE>(s, n, WS_ONE, val, part_start, part_start, w);
    switch (op) {
      case GPUQ_WIN_COUNT:
        win_slide_launch<SK_COUNT>(s, n, f64, val, lo, hi, part_start, w, out,
                                   out_validity_bits);
        break;
      case GPUQ_WIN_SUM:
        if (f64) win_slide_launch<SK_SUM_F64>(s, n, f64, val, lo, hi, part_start, w,
                                              out, out_validity_bits);
        else win_slide_launch<SK_SUM_U64>(s, n, f64, val, lo, hi, part_start, w, out,
                                          out_validity_bits);
        break;
      case GPUQ_WIN_MIN:
        win_slide_launch<SK_MIN>(s, n, f64, val, lo, hi, part_start, w, out,
                                 out_validity_bits);
        break;
      case GPUQ_WIN_MAX:
        win_slide_launch<SK_MAX>(s, n, f64, val, lo, hi, part_start, w, out,
                                 out_validity_bits);
        break;
      case GPUQ_WIN_FIRST_VALUE:
        win_slide_launch<SK_FIRST>(s, n, f64, val, lo, hi, part_start, w, out,
                                   out_validity_bits);
        break;
      default:
        win_slide_launch<SK_LAST>(s, n, f64, val, lo, hi, part_start, w, out,
                                  out_validity_bits);
        break;
    }
    HIP_TRY(hipGetLastError());
    return GPUQ_OK;
  }
  /* UNBOUNDED PRECEDING .. hi: an offset past either end of the input is past
   * every partition, and nrows rows ahead is UNBOUNDED FOLLOWING */
  if (hi > n) hi = n;
  if (hi < -n) hi = -n;
  const wu64* src = (const wu64*)val.data;
  const uint8_t* src_valid = val.validity;
  int mode = 0, never_null = 0;
  if (pick_val) {
    mode = op == GPUQ_WIN_FIRST_VALUE ? 1 : 2;
    win_reduce_carry<WK_NONE>(s, n, WS_ONE, val, part_start, part_start, w);
  } else {
    never_null = op == GPUQ_WIN_COUNT;
    src = tmp;
    src_valid = never_null ? nullptr : tmp_valid;
    switch (op) {
      case GPUQ_WIN_COUNT:
        win_scan_rows<WK_ADD_U64>(s, n, val.data ? WS_VALID : WS_ONE, val, part_start,
                                  part_start, w, 0, 1, tmp, nullptr);
        break;
      case GPUQ_WIN_SUM:
        if (f64) win_scan_rows<WK_ADD_F64>(s, n, WS_RAW, val, part_start, part_start,
                                           w, 0, 0, tmp, tmp_valid);
        else win_scan_rows<WK_ADD_U64>(s, n, WS_RAW, val, part_start, part_start, w,
                                       0, 0, tmp, tmp_valid);
        break;
      case GPUQ_WIN_MIN:
        win_scan_rows<WK_MIN>(s, n, f64 ? WS_ENC_F64 : WS_ENC_I64, val, part_start,
                              part_start, w, f64 ? 2 : 1, 0, tmp, tmp_valid);
        break;
      default:
        win_scan_rows<WK_MAX>(s, n, f64 ? WS_ENC_F64 : WS_ENC_I64, val, part_start,
                              part_start, w, f64 ? 2 : 1, 0, tmp, tmp_valid);
        break;
    }
  }
  HIP_TRY(hipGetLastError());
  { hipEvent_t _pe = prof_begin(s);
  k_win_pick<<<dim3((uint32_t)nt), WIN_BLOCK, 0, s>>>(
      n, mode, hi, src, src_valid, never_null, (const wu64*)part_start,
      w.prev_part, w.next_part, (wu64*)out, out_validity_bits, (n + 7) / 8);
  prof_end("win_pick", s, _pe); }
  HIP_TRY(hipGetLastError());
  return GPUQ_OK;
}
