// kernels.hip -- hand-written CDNA4 (gfx950) kernels of the ABFT sparse-CG hot
// path.  Everything here is HBM-bound integer/fp64 work: no MFMA; the levers
// are coalesced streaming of cols/vals, LDS-staged per-row partial products,
// XCD-aware tile order so each XCD's L2 keeps its own window of x, column
// panels for matrices whose gathers would otherwise miss L2, 64-lane wave
// reductions with a deterministic last-block fold, and the ECC check folded
// into the load path.  Design notes and the measurements behind each choice:
// DESIGN.md section 4.
//
// Numerics: compiled with -ffp-contract=off.  SpMV sums every row in ascending
// element order with separate multiply and add, so y is bit-identical to the
// reference CPUContext (CSR/CPUContext.cpp:115-133); calc_xr/calc_p are
// bit-identical element-wise; only the two reductions (tree order) differ from
// the reference's serial sums, in the last bits.
#include <type_traits>

#include "abft_internal.h"
#include "ecc_device.h"
#include "guard_protocol.h"
#include "matrix_digest.h"
#include "struct_ecc.h"
#include "trail_ecc.h"
#include "vecc_walk.h"

// native vector types (what __builtin_nontemporal_load accepts)
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#if ABFT_CFG_NT
#define STREAM_LOAD(p) __builtin_nontemporal_load(p)
#else
#define STREAM_LOAD(p) (*(p))
#endif

// how the x-gather is issued: 0 plain (through the CU's L1), 1 non-temporal, 2 sc1 (L1 bypass)
#ifndef ABFT_CFG_GATHER
#define ABFT_CFG_GATHER 0
#endif
__device__ __forceinline__ double gather_load(const double *p) {
#if ABFT_CFG_GATHER == 1
  return __builtin_nontemporal_load(p);
#elif ABFT_CFG_GATHER == 2
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// ------------------------------------------------------------------ helpers --

// Hardware deals consecutive workgroup ids round-robin over the 8 XCDs
// (MI355X_MICROARCH: blocks b and b+8 share one).  Give each XCD a contiguous
// range of tiles so the x-window its blocks gather from stays in that XCD's L2
// (speed only; the map is a bijection for every nblk).
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t nblk) {
#if ABFT_CFG_XCD == 0
  return b;
#elif ABFT_CFG_XCD == 2
  // chunked variant: the 8 XCDs share a window of 8*C consecutive tiles, each
  // taking C consecutive ones (keeps one HBM stream, still gives an XCD runs of
  // neighbouring tiles); the ragged tail keeps the identity map
  constexpr uint32_t C = ABFT_CFG_XCD_CHUNK;
  const uint32_t full = (nblk / (8u * C)) * (8u * C);
  if (b >= full) return b;
  const uint32_t g = b >> 3;
  return (g / C) * (8u * C) + (b & 7u) * C + g % C;
#endif
  const uint32_t xcd = b & 7u, q = nblk >> 3, r = nblk & 7u;
  const uint32_t first = xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
  return first + (b >> 3);
}

__device__ __forceinline__ void push_event(const EventRing &ev, uint32_t kind, uint32_t index,
                                           uint32_t bit, uint32_t fmt) {
  uint32_t slot = atomicAdd(ev.count, 1u);
  if (slot < ev.cap) {
    abft_event e;
    e.kind = kind; e.index = index; e.bit = bit; e.fmt = fmt;
    ev.buf[slot] = e;
  }
}

__device__ __forceinline__ double as_double(uint32_t lo, uint32_t hi) {
  return __hiloint2double((int)hi, (int)lo);
}

// Cold path of the ECC modes: the element failed its check.  Repairs `w` in
// place when the mode can and queues the event.  Returns 1 = repaired (caller
// writes the element back), -1 = fatal.
//   sed    reference CSR/CPUContext.cpp:230-235   COO/CPUContext.cpp:212-217
//   sec7   CSR :268-279                          COO :250-258
//   sec8   CSR :313-335                          COO :293-312
//   secded CSR :369-400                          COO :346-373
template <int FMT> struct EccWords { uint32_t w[EccLayout<FMT>::NW]; int rc; };

template <int FMT, int MODE>
__device__ __noinline__ EccWords<FMT> ecc_cold(EccWords<FMT> e, uint32_t gidx, EventRing ev) {
  constexpr int EW = EccLayout<FMT>::EW, NBITS = EccLayout<FMT>::NBITS;
  uint32_t *w = e.w;
  if (MODE == MODE_SED) {
    push_event(ev, ABFT_EV_SED_DETECTED, gidx, 0, FMT);
    e.rc = -1;
    return e;
  }
  const uint32_t h = ecc_hamming<FMT>(w);
  const uint32_t par = MODE == MODE_SEC7 ? 1u : ecc_parity<FMT>(w);
  if (par) {
    if (h) {
      const uint32_t bit = ecc_position_to_bit<FMT>(h);
      // static word selects keep the element in registers (no scratch array)
#pragma unroll
      for (int k = 0; k < EccLayout<FMT>::NW; k++)
        if ((bit >> 5) == (uint32_t)k) w[k] ^= 1u << (bit & 31u);
      (void)NBITS;  // bit >= NBITS (a mis-decoded multi-bit error) selects no word
      push_event(ev, ABFT_EV_CORRECTED_BIT, gidx, bit, FMT);
    } else {
      w[EW] ^= 1u << 24;
      push_event(ev, ABFT_EV_CORRECTED_PARITY, gidx, 0, FMT);
    }
    e.rc = 1;
    return e;
  }
  push_event(ev, ABFT_EV_DOUBLE_BIT, gidx, 0, FMT);  // parity even, syndrome set
  e.rc = -1;
  return e;
}

// the element index an event line carries: the caller's, global across shards
__device__ __forceinline__ uint32_t event_index_of_orig(const CsrDev &A, uint32_t o) {
  return A.gidx ? A.gidx[o] : A.index_base + o;
}
__device__ __forceinline__ uint32_t event_index(const CsrDev &A, uint32_t i) {
  return event_index_of_orig(A, A.orig_index ? A.orig_index[i] : i);
}
__device__ __forceinline__ uint32_t event_index(const CooDev &A, uint32_t j) {
  const uint32_t o = A.orig_index[j];
  return A.gidx ? A.gidx[o] : A.index_base + o;
}

// Hot-path test: non-zero iff the element needs the cold path.
template <int FMT, int MODE>
__device__ __forceinline__ uint32_t ecc_suspect(const uint32_t *w) {
  if (MODE == MODE_SED || MODE == MODE_SEC8) return ecc_parity<FMT>(w);  // sec8 is lazy
  if (MODE == MODE_SEC7) return ecc_any_check<FMT>(w);
  if (MODE == MODE_SECDED) return ecc_any_check<FMT>(w) | ecc_parity<FMT>(w);
  return 0;
}

// ---- protected vector elements (ecc_device.h "protected vector elements") ----
// Cold path: the word failed vecc_suspect.  vecc_repair (ecc_device.h) repairs what it can, here the outcome is
// reported: rc 1 a flipped bit put back, rc -1 two flips, fatal, the word as it is.  `operand`: the vector's
// ordinal in the entry's argument list, `index` the element inside it.
//
// A vector entry may be read by any number of threads -- every row of a dense column gathers the same
// x[col] -- and each of them comes here with the same damaged word.  All repair it in their registers, but
// only the first queues the event: a flipped word costs one slot of the queue however many threads see
// it (65536 gatherers of one flipped bit would otherwise overflow the queue and end the solve, with y
// correct).  The "already queued" table lies behind the ring's `cap` events (abft_internal.h): open
// addressing over 64-bit keys {kind, index, bit | operand << 8} -- never 0, kind >= 10 --, cleared by the
// drain.  A thread that meets only foreign keys queues its event anyway; the drain drops what still
// repeats.
__device__ __forceinline__ void push_vector_event(const EventRing &ev, uint32_t kind, uint32_t index, uint32_t bit) {
  const unsigned long long key = ((unsigned long long)kind << 48) | ((unsigned long long)index << 16) |
                                 (unsigned long long)(bit & 0xffffu);
  unsigned long long *seen = reinterpret_cast<unsigned long long *>(ev.buf + ev.cap);
  uint32_t h = ((index + (bit << 12)) * 0x9E3779B1u) >> 20;  // (32-bit: the callers' registers are this function's)
#pragma unroll 1
  for (uint32_t k = 0; k < ABFT_VECC_SEEN_PROBES; k++, h++) {
    const unsigned long long was = atomicCAS(seen + (h & (ABFT_VECC_SEEN_SLOTS - 1u)), 0ull, key);
    if (was == key) return;  // queued by another thread
    if (was == 0ull) break;  // ours now
  }
  push_event(ev, kind, index, bit, ABFT_FMT_VECTOR);
}

__device__ __noinline__ VeccWord vecc_cold(uint64_t word, uint32_t index, uint32_t operand, EventRing ev) {
  VeccWord o;
  uint32_t bit;
  vecc_repair(word, o, bit);
  if (o.rc) push_vector_event(ev, o.rc > 0 ? ABFT_EV_VEC_CORRECTED : ABFT_EV_VEC_DOUBLE, index, bit | (operand << 8));
  return o;
}

// the cold decode as the walks of vecc_walk.h take it
struct VeccColdDev {
  EventRing ev;
  __device__ __forceinline__ VeccWord operator()(uint64_t word, uint32_t index, uint32_t operand) const {
    return vecc_cold(word, index, operand, ev);
  }
};

// full decode of one word outside any load loop: check, repair in registers, event
__device__ __forceinline__ double vecc_decode_cold_ok(const double *p, uint32_t index, uint32_t operand,
                                                      const EventRing &ev) {
  uint64_t w = vecc_bits(*p);
  if (__builtin_expect(vecc_suspect(w) != 0u, 0)) w = vecc_cold(w, index, operand, ev).w;
  return vecc_value(w);
}

// The protected SpMV's gathers: the gathered words -> the values to multiply with; bit j of the result is
// set when entry j failed its check.  As for the matrix elements (csr_consume), a failing entry is only
// NOTED here ...
template <int EPT>
__device__ __forceinline__ uint32_t vecc_decode_gathers(double *xv) {
  uint32_t xbad = 0u;
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const uint64_t w = vecc_bits(xv[j]);
    xbad |= vecc_suspect(w) << j;
    xv[j] = vecc_value(w);
  }
  return xbad;
}

// ... and behind the tile's LDS writes the noted entries are read again, repaired in registers by
// vecc_cold (the vector is not written back: many threads gather the same entry, and the kernel that
// next rewrites it repairs it) and their products staged anew.  Unrolled with static selects, so col
// and val stay in registers.
template <int EPT>
__device__ __forceinline__ void vecc_redo_gathers(uint32_t xbad, const double *__restrict__ x, const uint32_t *col,
                                                  const double *val, const EventRing &ev, double *s_prod) {
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    if ((xbad >> j) & 1u) {
      const VeccWord r = vecc_cold(vecc_bits(x[col[j]]), col[j], 0u, ev);
      s_prod[2u * threadIdx.x + (uint32_t)(j >> 1) * (2u * ABFT_BLOCK) + (uint32_t)(j & 1)] = val[j] * vecc_value(r.w);
    }
  }
}

// One step of a cross-lane reduction on the DPP path (the operand is permuted
// inside the VALU, nothing goes through LDS): lanes whose source is out of range
// or whose row is masked off read 0.0.  __shfl_down on a double compiles to two
// ds_bpermute_b32 + a wait per step; six dependent steps of that in an epilogue
// kept every SpMV workgroup alive ~0.3 us longer.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
  return __hiloint2double(hi, lo);
}

// sum over the 64 lanes in a fixed tree; the total is valid in LANE 63 only
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0x111, 0xf>(v);  // row_shr:1
  v += dpp_f64<0x112, 0xf>(v);  // row_shr:2
  v += dpp_f64<0x114, 0xf>(v);  // row_shr:4
  v += dpp_f64<0x118, 0xf>(v);  // row_shr:8  -> lane 15 of each 16-lane row holds the row's sum
  v += dpp_f64<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v += dpp_f64<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds all 64
  return v;
}

// fixed-shape block reduction (256 threads = 4 waves); every thread gets the sum
__device__ __forceinline__ double block_sum(double v, double *s_w) {
  v = wave_sum(v);
  if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// --------------------------------------------------------------- ECC encode --

// create_matrix's per-element encode (reference CSR/CPUContext.cpp:25-35)
__global__ __launch_bounds__(ABFT_BLOCK) void encode_csr_kernel(int mode, uint32_t *cols,
                                                                double *vals, uint32_t nnz) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += gridDim.x * blockDim.x) {
    const double v = vals[i];
    uint32_t w[3] = {(uint32_t)__double2loint(v), (uint32_t)__double2hiint(v), cols[i]};
    ecc_encode<FMT_CSR>(mode, w);
    cols[i] = w[2];
  }
}

// reference COO/CPUContext.cpp:22-33
__global__ __launch_bounds__(ABFT_BLOCK) void encode_coo_kernel(int mode, uint4 *elems, uint32_t nnz) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += gridDim.x * blockDim.x) {
    uint4 e = elems[i];
    uint32_t w[4] = {e.x, e.y, e.z, e.w};
    ecc_encode<FMT_COO>(mode, w);
    e.x = w[0];
    elems[i] = e;
  }
}

hipError_t launch_encode_csr(int mode, uint32_t *cols, double *vals, uint32_t nnz, hipStream_t s) {
  if (!nnz || mode < MODE_SED) return hipSuccess;
  uint32_t grid = (nnz + ABFT_BLOCK - 1) / ABFT_BLOCK;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(encode_csr_kernel, dim3(grid), dim3(ABFT_BLOCK), 0, s, mode, cols, vals, nnz);
  return hipGetLastError();
}
hipError_t launch_encode_coo(int mode, uint4 *elems, uint32_t nnz, hipStream_t s) {
  if (!nnz || mode < MODE_SED) return hipSuccess;
  uint32_t grid = (nnz + ABFT_BLOCK - 1) / ABFT_BLOCK;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(encode_coo_kernel, dim3(grid), dim3(ABFT_BLOCK), 0, s, mode, elems, nnz);
  return hipGetLastError();
}

// ---------------------------------------------- COO fix-up (defined further down) --

__device__ void coo_fixup_body(const FixArgs &fx);

// ------------------------------------------------------ fused dot epilogue --

// All-reduce of {v0, v1} (held by thread 0) across the ranks of a peer board, by every thread
// of the calling block: see peer_allreduce_kernel below for the protocol.  Thread 0 returns
// the sums in rank order; a rank that gives up waiting gets NaN and raises its flag.
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// Accesses to the shared region that go to memory whatever the caches hold (sc0 sc1: system
// coherence level), 16 bytes wide: the compiler has no 16-byte system-scope atomic, and 8-byte
// ones cross the link one request per lane.  No fences anywhere in this kernel -- a system-scope
// release writes back every dirty line of the XCD's L2 first (the vectors the iteration has just
// written) -- the order comes from waiting for the stores (vmcnt) before the flag is stored.
__device__ __forceinline__ void sys_store_b128(u64x2 *p, u64x2 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void sys_store_b64(unsigned long long *p, unsigned long long v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void sys_load4_b128(const u64x2 *p0, const u64x2 *p1, const u64x2 *p2, const u64x2 *p3,
                                               u64x2 &w0, u64x2 &w1, u64x2 &w2, u64x2 &w3) {
  asm volatile(
      "global_load_dwordx4 %0, %4, off sc0 sc1\n\t"
      "global_load_dwordx4 %1, %5, off sc0 sc1\n\t"
      "global_load_dwordx4 %2, %6, off sc0 sc1\n\t"
      "global_load_dwordx4 %3, %7, off sc0 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3)
      : "v"(p0), "v"(p1), "v"(p2), "v"(p3)
      : "memory");
}
__device__ __forceinline__ void sys_load2_b128(const u64x2 *p0, const u64x2 *p1, u64x2 &w0, u64x2 &w1) {
  asm volatile(
      "global_load_dwordx4 %0, %2, off sc0 sc1\n\t"
      "global_load_dwordx4 %1, %3, off sc0 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(w0), "=&v"(w1)
      : "v"(p0), "v"(p1)
      : "memory");
}
__device__ __forceinline__ unsigned long long sys_load_b64(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ unsigned long long peer_check_word(unsigned long long seq, double v0, double v1) {
  return (seq * 0x9E3779B97F4A7C15ull) ^ (unsigned long long)__double_as_longlong(v0) ^
         ((unsigned long long)__double_as_longlong(v1) << 1 | (unsigned long long)__double_as_longlong(v1) >> 63);
}

// `seq_given` != 0: the caller names the sequence number and says whether this call leaves it in the counter
// (cg_tail_kernel: two all-reduces in one launch, run by different workgroups -- a counter bumped by the first
// would sit dirty in that workgroup's L2 when the second reads it)
// `publish` false: this workgroup only READS the ranks' slots (every workgroup of cg_tail_kernel forms the sum itself;
// one of them publishes this rank's slot).
__device__ __forceinline__ void peer_allreduce_block(double &v0, double &v1, const PeerArgs &P,
                                                     unsigned long long seq_given = 0ull, bool write_counter = true,
                                                     bool publish = true) {
  __shared__ double s_pv[2][ABFT_PEER_MAX_RANKS];
  __shared__ double s_mine[2];
  __shared__ unsigned long long s_pseq;
  __shared__ uint32_t s_pbad;
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    const unsigned long long seq = seq_given ? seq_given : *P.counter + 1ull;  // (counter: written by the previous all-reduce on this stream)
    if (!P.boards && publish) {
      PeerSlot *mine = P.board + (size_t)(seq & 1ull) * ABFT_PEER_MAX_RANKS + P.rank;
      // two 16-byte stores, {v0, v1} and {sequence number, check word}, not waited for and in no
      // particular order: a reader takes a slot only when its check word fits the sequence number AND
      // the values next to it, so it cannot pair a new number with an old value; it polls whole slots,
      // which makes an all-reduce one store and (mostly) one load across the link instead of a store,
      // its acknowledgement, a flag, a poll and a load
      u64x2 *half = reinterpret_cast<u64x2 *>(mine);
      sys_store_b128(half, u64x2{(unsigned long long)__double_as_longlong(v0), (unsigned long long)__double_as_longlong(v1)});
      sys_store_b128(half + 1, u64x2{seq, peer_check_word(seq, v0, v1)});
    }
    s_mine[0] = v0;
    s_mine[1] = v1;
    s_pseq = seq;
    s_pbad = 0u;
  }
  __syncthreads();
  const unsigned long long seq = s_pseq;
  // Replicated board (device memory, one copy per rank, the peers' copies mapped over IPC): lane r
  // PUSHES this rank's slot into rank r's copy -- remote stores, which the fabric posts -- and every
  // rank polls only its OWN copy, in its own memory.  Same slot format, same check word.
  const PeerSlot *poll = P.board;
  if (P.boards) {
    if (publish && t < (uint32_t)P.size) {
      const double m0 = s_mine[0], m1 = s_mine[1];
      u64x2 *half = reinterpret_cast<u64x2 *>(P.boards[t] + (size_t)(seq & 1ull) * ABFT_PEER_MAX_RANKS + P.rank);
      sys_store_b128(half, u64x2{(unsigned long long)__double_as_longlong(m0), (unsigned long long)__double_as_longlong(m1)});
      sys_store_b128(half + 1, u64x2{seq, peer_check_word(seq, m0, m1)});
    }
    poll = P.boards[P.rank];
  }
  if (t < (uint32_t)P.size) {
    const u64x2 *half = reinterpret_cast<const u64x2 *>(poll + (size_t)(seq & 1ull) * ABFT_PEER_MAX_RANKS + t);
    const unsigned long long t0 = (unsigned long long)wall_clock64();
    bool ok = false;
    double a = 0.0, b = 0.0;
    for (;;) {
      u64x2 val, tag;
      sys_load2_b128(half, half + 1, val, tag);
      a = __longlong_as_double((long long)val.x);
      b = __longlong_as_double((long long)val.y);
      if (tag.x == seq && tag.y == peer_check_word(seq, a, b)) {
        ok = true;
        break;
      }
      if ((unsigned long long)wall_clock64() - t0 > P.timeout_ticks) break;
      __builtin_amdgcn_s_sleep(2);
    }
    if (!ok) {
      a = b = 0.0;
      atomicOr(&s_pbad, 1u);
    }
    s_pv[0][t] = a;
    s_pv[1][t] = b;
  }
  __syncthreads();
  if (t == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int r = 0; r < P.size; r++) {
      s0 += s_pv[0][r];
      s1 += s_pv[1][r];
    }
    if (s_pbad) {
      s0 = __longlong_as_double(0x7ff8000000000000ll);
      __hip_atomic_store(P.fail + P.rank, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    v0 = s0;
    v1 = s1;
    if (write_counter) *P.counter = seq;
  }
}


// Tail of an SpMV launched with a FuseOut: `dsum` is this thread's share of
// sum vec[row]*result[row].  The block leaves one partial with a plain store
// and exits -- nothing here waits on memory.  (An in-kernel ticket protocol
// was measured first: the storing lane's drain + returning atomic kept every
// block resident ~2x longer and cost 75 us per SpMV.)  A fold kernel (fuse_finalize_kernel
// below, or fold_partials_kernel when there are many partials),
// launched behind the SpMV on the same stream, folds the partials in a fixed
// order and publishes the scalar.
__device__ __forceinline__ void fused_dot_finish(double dsum, const FuseOut &f, uint32_t slot) {
  __shared__ double s_w[4];
  const double bsum = block_sum(dsum, s_w);
  if (threadIdx.x == 0) f.partials[slot] = bsum;
}

__global__ __launch_bounds__(1024) void fuse_finalize_kernel(FuseOut f, uint32_t nblk, FixArgs fx) {
  __shared__ double s_w[16];
  if (fx.on) coo_fixup_body(fx);  // COO: moved products first (it corrects partial 0); returns at once on clean data
  // fixed order; sixteen independent loads in flight per thread
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < nblk; i += 16u * 1024u) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const uint32_t j = i + (uint32_t)k * 1024u;
      v[k] = j < nblk ? f.partials[j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 16; k += 4) acc += (v[k] + v[k + 1]) + (v[k + 2] + v[k + 3]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  double tot = 0.0, evs = 0.0;
  uint32_t nev = 0u;
  if (threadIdx.x == 0) {
    for (int k = 0; k < 16; k++) tot += s_w[k];
    nev = *f.ev_count;
    evs = (double)nev;
  }
  if (f.peers.size) peer_allreduce_block(tot, evs, f.peers);  // (uniform: a kernel argument)
  if (threadIdx.x == 0) {
    if (f.dev_out) {
      f.dev_out[0] = tot;
      f.dev_out[1] = evs;
    }
    if (f.host) {
      __hip_atomic_store(&f.host->value, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&f.host->evcount, nev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&f.host->seq, f.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}


// ----------------------------------------------------------------- CSR SpMV --

// Load phase of one tile: elements [lo, hi) of the matrix, staged at LDS slot
// (i - base); base is even so every thread's pair load is 16-byte aligned and a
// wave instruction streams 1 KiB of vals / 512 B of cols, contiguous.
//
// Written branch-free on purpose: every lane issues all its loads (an
// out-of-tile lane re-reads the tile's first pair), then all its gathers
// (index clamped to 0 when out of range), then multiplies and selects.  With
// per-element `if`s hipcc puts an s_waitcnt vmcnt(0) at every join and the four
// gathers of a thread run one after the other.  The only branch left is the
// ECC cold path, taken when an element fails its check.
template <int EPT> struct CsrTileRegs {
  f64x2 v[EPT / 2];
  u32x2 c[EPT / 2];
};

// the streaming loads of one tile: no branches, out-of-tile lanes re-read the first pair
template <int EPT>
__device__ __forceinline__ void csr_issue_loads(const CsrDev &A, uint32_t base, uint32_t hi,
                                                CsrTileRegs<EPT> &t) {
#pragma unroll
  for (int s = 0; s < EPT / 2; s++) {
    const uint32_t i = base + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK);
    const uint32_t ii = i < hi ? i : base;  // always a valid, even element index
    t.v[s] = STREAM_LOAD(reinterpret_cast<const f64x2 *>(A.vals + ii));
    t.c[s] = STREAM_LOAD(reinterpret_cast<const u32x2 *>(A.cols + ii));
  }
#if ABFT_CFG_SCHED_BARRIER
  // keep every streaming load ahead of the first wait: left alone, hipcc sinks half of
  // the value loads below the gathers, where they start one HBM latency late
  __builtin_amdgcn_sched_barrier(0);
#endif
}

// ECC check, gathers, products -> LDS for a tile whose loads were issued into
// `t`.  If `prefetch`, the NEXT tile's streaming loads are issued right after
// this tile's gathers (so the gathers stay older in the memory queue and can be
// waited for without draining the prefetch).  A persistent, software-pipelined
// kernel built on this was measured and dropped: 180 us vs 151 us for one tile
// per workgroup (config 2) -- 8 resident workgroups per CU already overlap each
// other's phases, and the extra registers cost occupancy.
template <int MODE, int EPT, bool VECC = false>
__device__ __forceinline__ void csr_consume(const CsrDev &A, const double *__restrict__ x,
                                            const EventRing &ev, uint32_t base, uint32_t lo,
                                            uint32_t hi, const CsrTileRegs<EPT> &t, double *s_prod,
                                            uint32_t *s_col, bool prefetch, uint32_t nbase, uint32_t nhi,
                                            CsrTileRegs<EPT> &nxt) {
  constexpr int STEPS = EPT / 2;
  uint32_t col[EPT];
  double val[EPT];
  bool ok[EPT];
  uint32_t bad = 0u;  // bit j: element j of this lane failed its ECC check
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const int s = j >> 1;
    const uint32_t i = base + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK) + (uint32_t)(j & 1);
    const double d = (j & 1) ? t.v[s].y : t.v[s].x;
    uint32_t w[3] = {(uint32_t)__double2loint(d), (uint32_t)__double2hiint(d), (j & 1) ? t.c[s].y : t.c[s].x};
    bool valid = i >= lo && i < hi;
    if (MODE >= MODE_SED) {
      // An element that fails its check is only NOTED here; ecc_cold -- out of line -- runs behind the LDS writes
      // (below), where nothing of the tile is live.  With the call inside this loop hipcc has to assume at every join
      // behind it that the memory counters are unknown: config 4 secded 660 us against 632 for a timing build
      // without the call, config 2 secded 145.4 against 141.8 (profiles/r04/nocold_ab.txt).
      if (valid && ecc_suspect<FMT_CSR, MODE>(w) != 0) bad |= 1u << j;
      w[2] &= ABFT_COLMASK;  // reference CSR/CPUContext.cpp:238, 282, 338, 404
    }
    col[j] = w[2];
    val[j] = as_double(w[0], w[1]);
    ok[j] = valid;
  }
  double xv[EPT];
  // (Measured and dropped: scheduling barriers around this loop so that all gathers of the tile go out
  // before the first is used.  Left alone hipcc issues them one at a time in the sweep kernel with 8 and
  // 16 rows per thread, each behind an s_waitcnt vmcnt(0) for the one before -- and that is the faster
  // form there: 667 vs 745 us on config 4 with 16 rows per thread, 689 vs 675 with 8, no difference on
  // the streaming kernel -- and pinned in groups of 1, 2 or 4 it is 754 us all the same: what the barriers
  // take away is the compiler's interleaving of one element's gather with the next element's checks.)
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const bool in = ok[j] && col[j] < A.n_in;  // a corrupted index must never fault the GPU
#ifdef ABFT_DBG_NOGATHER  // timing-only build: wrong results
    xv[j] = (double)col[j];
#else
    xv[j] = gather_load(x + (in ? col[j] : 0u));
#endif
    if (!in) xv[j] = 0.0;
  }
  uint32_t xbad = 0u;  // VECC: bit j: the gathered entry of element j failed its check
  if (VECC) xbad = vecc_decode_gathers<EPT>(xv) & ~bad;  // (an element noted in `bad` gathers again below)
  // no branch around the prefetch: with one, hipcc drains the whole memory queue
  // (vmcnt(0)) at the join and the overlap is gone; a caller with nothing to
  // prefetch passes nhi == nbase, which makes every lane re-read one resident pair
  if (prefetch) csr_issue_loads<EPT>(A, nbase, nhi, nxt);
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const uint32_t k = 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK);
    const double p0 = val[2 * s] * xv[2 * s], p1 = val[2 * s + 1] * xv[2 * s + 1];
    *reinterpret_cast<double2 *>(s_prod + k) = make_double2(ok[2 * s] ? p0 : 0.0, ok[2 * s + 1] ? p1 : 0.0);
    if (MODE == MODE_CONSTRAINTS)
      *reinterpret_cast<uint2 *>(s_col + k) = make_uint2(col[2 * s], col[2 * s + 1]);
  }
  if (VECC && __builtin_expect(xbad != 0u, 0)) vecc_redo_gathers<EPT>(xbad, x, col, val, ev, s_prod);
#ifndef ABFT_DBG_NOCOLD  // (timing-only build without the repairs: wrong results for an element that fails its check)
  if (MODE >= MODE_SED && __builtin_expect(bad != 0u, 0)) {
    // the noted elements again, from memory: repaired (and written back: reference CSR/CPUContext.cpp:275-276,
    // 333-334, 389-390) or given up (fatal: the reference never uses the element), their product staged anew
#pragma unroll 1
    for (uint32_t j = 0; j < (uint32_t)EPT; j++) {
      if (!((bad >> j) & 1u)) continue;
      const uint32_t i = base + 2u * threadIdx.x + (j >> 1) * (2u * ABFT_BLOCK) + (j & 1u);
      const double d = A.vals[i];
      EccWords<FMT_CSR> e;
      e.w[0] = (uint32_t)__double2loint(d); e.w[1] = (uint32_t)__double2hiint(d); e.w[2] = A.cols[i]; e.rc = 0;
      e = ecc_cold<FMT_CSR, MODE>(e, event_index(A, i), ev);
      double p = 0.0;
      if (e.rc > 0) {
        A.vals[i] = as_double(e.w[0], e.w[1]);
        A.cols[i] = e.w[2];
        const uint32_t c = e.w[2] & ABFT_COLMASK;  // reference CSR/CPUContext.cpp:238, 282, 338, 404
#ifdef ABFT_DBG_NOGATHER
        p = as_double(e.w[0], e.w[1]) * (double)c;
#else
        if (VECC)
          p = as_double(e.w[0], e.w[1]) * (c < A.n_in ? vecc_decode_cold_ok(x + c, c, 0u, ev) : 0.0);
        else
          p = as_double(e.w[0], e.w[1]) * (c < A.n_in ? gather_load(x + c) : 0.0);
#endif
      }
      s_prod[i - base] = p;
    }
  }
#endif
}

// load + consume of one tile (the non-pipelined form)
template <int MODE, int EPT, bool VECC = false>
__device__ __forceinline__ void csr_stage(const CsrDev &A, const double *__restrict__ x,
                                          const EventRing &ev, uint32_t base, uint32_t lo,
                                          uint32_t hi, double *s_prod, uint32_t *s_col) {
  CsrTileRegs<EPT> t, unused;
  csr_issue_loads<EPT>(A, base, hi, t);
  csr_consume<MODE, EPT, VECC>(A, x, ev, base, lo, hi, t, s_prod, s_col, false, 0u, 0u, unused);
}

// Mode none, one tile (see CsrCompact): the loads of csr_stage, with the column source chosen per
// workgroup -- for a compact tile (cb != ABFT_CBASE_WIDE) the u16 offsets from the block's base
// `cb`, 2 bytes per element instead of 4, else the u32 columns.  Branch-free like csr_issue_loads:
// each step issues ONE 8-byte column load either way, from a uniformly selected address (compact:
// the lane's two offsets in its low dword; the high dword, the next lane's pair, is not used --
// cols16 is padded for it, and a wave's column loads still cover one contiguous run of 260 bytes).
// A branch into two staged paths was tried first and dropped on its ISA: hipcc hoisted the value
// loads above the branch and rejoined the paths before the gathers, so the wait for the columns
// also drained the value loads.  When e0 is odd, slot `base` holds the previous block's element, whose offset is
// relative to that block's base: it is masked invalid, as in csr_stage.
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
template <int EPT, bool VECC = false>
__device__ __forceinline__ void csr_stage_none(const CsrDev &A, const CsrCompact &cc, uint32_t cb,
                                               const double *__restrict__ x, const EventRing &ev, uint32_t base,
                                               uint32_t lo, uint32_t hi, double *s_prod, uint32_t *s_col) {
  const bool compact = cb != ABFT_CBASE_WIDE;  // workgroup-uniform
  CsrTileRegs<EPT> t, unused;
  u32x2 raw[EPT / 2];
  uint32_t ii[EPT / 2];
  // the column loads first: the gathers wait for them only, not for the value loads behind them
#pragma unroll
  for (int s = 0; s < EPT / 2; s++) {
    const uint32_t i = base + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK);
    ii[s] = i < hi ? i : base;  // always a valid, even element index
    const u32x2_a4 *pc = compact ? reinterpret_cast<const u32x2_a4 *>(cc.cols16 + ii[s])
                                 : reinterpret_cast<const u32x2_a4 *>(A.cols + ii[s]);
    raw[s] = STREAM_LOAD(pc);
  }
#pragma unroll
  for (int s = 0; s < EPT / 2; s++) t.v[s] = STREAM_LOAD(reinterpret_cast<const f64x2 *>(A.vals + ii[s]));
#if ABFT_CFG_SCHED_BARRIER
  __builtin_amdgcn_sched_barrier(0);  // as in csr_issue_loads; the offsets are widened behind it
#endif
#pragma unroll
  for (int s = 0; s < EPT / 2; s++) {
    t.c[s].x = compact ? cb + (raw[s].x & 0xFFFFu) : raw[s].x;
    t.c[s].y = compact ? cb + (raw[s].x >> 16) : raw[s].y;
  }
  csr_consume<MODE_NONE, EPT, VECC>(A, x, ev, base, lo, hi, t, s_prod, s_col, false, 0u, 0u, unused);
}

// Mode none, one packed tile (see CsrPacked): the only streamed load is the u16 code, one dword
// (two codes) per step at the slots csr_stage uses, so the LDS layout and everything behind the
// barrier stay as they are.  The palette is wave-held: lane l loads entry l & 15 (an L2 hit: the
// pool is a few hundred bytes), and each element's value comes from the lane its index names by
// ds_bpermute -- no LDS traffic, no barrier, no select chain.  The product is the same v_mul_f64
// of the same two operands as csr_consume's, so y is bit-identical.  The slot before e0 (odd e0)
// holds the previous block's code: masked invalid like in csr_stage; its index reads this
// block's palette all the same (padded to 16 entries) and its column gathers nothing.
template <int EPT, bool VECC = false>
__device__ __forceinline__ void csr_stage_packed(const CsrDev &A, const CsrPacked &cp, uint2 pd,
                                                 const double *__restrict__ x, const EventRing &ev, uint32_t base,
                                                 uint32_t lo, uint32_t hi, double *s_prod) {
  constexpr int STEPS = EPT / 2;
  const uint32_t shift = pd.y & 31u, mask = (1u << shift) - 1u;  // uniform
  const uint32_t pbase = (pd.y >> 5) * ABFT_PAL_ENTRIES;
#if ABFT_CFG_PACKED_PAL == 0
  const double pal = cp.pal[pbase + (threadIdx.x & (ABFT_PAL_ENTRIES - 1u))];
  const int pal_lo = __double2loint(pal), pal_hi = __double2hiint(pal);
#elif ABFT_CFG_PACKED_PAL == 1
  double pal[ABFT_PAL_ENTRIES];  // uniform: scalar loads
#pragma unroll
  for (uint32_t e = 0; e < ABFT_PAL_ENTRIES; e++) pal[e] = cp.pal[pbase + e];
#endif
  uint32_t raw[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const uint32_t i = base + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK);
    const uint32_t ii = i < hi ? i : base;  // always a valid, even element index
    raw[s] = STREAM_LOAD(reinterpret_cast<const uint32_t *>(cp.code16 + ii));
  }
  uint32_t col[EPT];
  double val[EPT];
  bool ok[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const int s = j >> 1;
    const uint32_t i = base + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK) + (uint32_t)(j & 1);
    const uint32_t code = (j & 1) ? raw[s] >> 16 : raw[s] & 0xFFFFu;
    const uint32_t idx = code >> shift;  // <= 15
    col[j] = pd.x + (code & mask);
#if ABFT_CFG_PACKED_PAL == 0
    const int src = (int)(idx << 2);  // byte address of the palette lane
    val[j] = as_double((uint32_t)__builtin_amdgcn_ds_bpermute(src, pal_lo),
                       (uint32_t)__builtin_amdgcn_ds_bpermute(src, pal_hi));
#elif ABFT_CFG_PACKED_PAL == 1
    double l1[8], l2[4], l3[2];  // select tree on the index bits
#pragma unroll
    for (int e = 0; e < 8; e++) l1[e] = (idx & 1u) ? pal[2 * e + 1] : pal[2 * e];
#pragma unroll
    for (int e = 0; e < 4; e++) l2[e] = (idx & 2u) ? l1[2 * e + 1] : l1[2 * e];
#pragma unroll
    for (int e = 0; e < 2; e++) l3[e] = (idx & 4u) ? l2[2 * e + 1] : l2[2 * e];
    val[j] = (idx & 8u) ? l3[1] : l3[0];
#else
    val[j] = cp.pal[pbase + idx];  // a per-lane load of the (cache-resident) palette
#endif
    ok[j] = i >= lo && i < hi;
  }
  double xv[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const bool in = ok[j] && col[j] < A.n_in;  // a corrupted index must never fault the GPU
    xv[j] = gather_load(x + (in ? col[j] : 0u));
    if (!in) xv[j] = 0.0;
  }
  uint32_t xbad = 0u;
  if (VECC) xbad = vecc_decode_gathers<EPT>(xv);
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const uint32_t k = 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK);
    const double p0 = val[2 * s] * xv[2 * s], p1 = val[2 * s + 1] * xv[2 * s + 1];
    *reinterpret_cast<double2 *>(s_prod + k) = make_double2(ok[2 * s] ? p0 : 0.0, ok[2 * s + 1] ? p1 : 0.0);
  }
  if (VECC && __builtin_expect(xbad != 0u, 0)) vecc_redo_gathers<EPT>(xbad, x, col, val, ev, s_prod);
}

// csr_stage_packed on a block whose fast word (CsrPackedFast) has the stage bit: the planner has proven that the
// whole tile window of codes is allocated and that every 16-bit code decodes to a column inside x, so the code
// loads are not clamped, the gathers not tested and nothing is zeroed -- no compare, no select.  The slots outside
// [e0, e1) (the one before an odd e0, those behind e1) stage a product of whatever code lies there: finite
// garbage or not, no row's range reads it.  Inside [e0, e1): the same v_mul_f64 of the same two operands.
// ABFT_CFG_PACKED_PAL == 0 only (the caller falls back to csr_stage_packed otherwise).
template <int EPT>
__device__ __forceinline__ void csr_stage_packed_fast(const CsrPacked &cp, uint2 pd, const double *__restrict__ x,
                                                      uint32_t base, double *s_prod) {
  constexpr int STEPS = EPT / 2;
  const uint32_t shift = pd.y & 31u, mask = (1u << shift) - 1u;  // uniform
  const uint32_t pbase = (pd.y >> 5) * ABFT_PAL_ENTRIES;
  const double pal = cp.pal[pbase + (threadIdx.x & (ABFT_PAL_ENTRIES - 1u))];
  const int pal_lo = __double2loint(pal), pal_hi = __double2hiint(pal);
  const double *xb = x + pd.x;  // uniform
  uint32_t raw[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; s++)
    raw[s] = STREAM_LOAD(reinterpret_cast<const uint32_t *>(cp.code16 + base + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK)));
  double xv[EPT], val[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const uint32_t code = (j & 1) ? raw[j >> 1] >> 16 : raw[j >> 1] & 0xFFFFu;
    xv[j] = gather_load(xb + (code & mask));
    const int src = (int)((code >> shift) << 2);  // byte address of the palette lane
    val[j] = as_double((uint32_t)__builtin_amdgcn_ds_bpermute(src, pal_lo),
                       (uint32_t)__builtin_amdgcn_ds_bpermute(src, pal_hi));
  }
#pragma unroll
  for (int s = 0; s < STEPS; s++)
    *reinterpret_cast<double2 *>(s_prod + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK)) =
        make_double2(val[2 * s] * xv[2 * s], val[2 * s + 1] * xv[2 * s + 1]);
}

// The row phase of a block whose fast word carries a row length: LEN products from p[0], added in ascending order
// onto 0.0 -- the first add is kept (0.0 + a0: what turns a lone -0.0 product into +0.0 in csr_row_sum too).  All
// reads are issued before the first add; the offsets are immediates.
template <int LEN>
__device__ __forceinline__ double csr_row_sum_fixed(const double *p) {
  double a[LEN];
#pragma unroll
  for (int j = 0; j < LEN; j++) a[j] = p[j];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < LEN; j++) acc += a[j];
  return acc;
}
__device__ __forceinline__ double csr_row_sum_len(const double *p, uint32_t len) {  // len: uniform, 1 .. ABFT_FAST_LEN_MAX
  switch (len) {
    case 1: return csr_row_sum_fixed<1>(p);
    case 2: return csr_row_sum_fixed<2>(p);
    case 3: return csr_row_sum_fixed<3>(p);
    case 4: return csr_row_sum_fixed<4>(p);
    case 5: return csr_row_sum_fixed<5>(p);
    case 6: return csr_row_sum_fixed<6>(p);
    case 7: return csr_row_sum_fixed<7>(p);
    default: return csr_row_sum_fixed<8>(p);
  }
}

// Constraints mode: the reference's two checks of element i (CSR/CPUContext.cpp:186-200) on
// the staged columns -- its column against the vector's size, then against its row successor's
// (read from the matrix when element i is the last one staged).  Returns false if a fatal event
// was queued.  (csr_row_sum and the block SpMV, spmm_row_sum, run the same checks.)
__device__ __forceinline__ bool csr_check_element(const CsrDev &A, const EventRing &ev, uint32_t base, uint32_t i,
                                                  uint32_t re, uint32_t row_end, const uint32_t *s_col,
                                                  uint32_t row) {
  const uint32_t k = i - base;
  const uint32_t col = s_col[k];
  if (col >= A.n_in) {
    push_event(ev, ABFT_EV_COL_SIZE, A.index_base + i, row, FMT_CSR);  // `bit` = row: the drain's sort key
    return false;
  }
  if (i + 1u < row_end) {
    // the next column is in the tile unless this is the last staged element
    const uint32_t nxt = (i + 1u < re) ? s_col[k + 1u] : A.cols[i + 1u];
    if (nxt <= col) {
      push_event(ev, ABFT_EV_COL_ORDER, A.index_base + i, row, FMT_CSR);
      return false;
    }
  }
  return true;
}

// Sum one row from the staged products, in ascending element order.  In
// constraints mode also runs the reference's structural checks in that order
// (CSR/CPUContext.cpp:186-200).  Returns false if a fatal event was queued.
template <int MODE, bool SHORT = false>
__device__ __forceinline__ bool csr_row_sum(const CsrDev &A, const EventRing &ev, uint32_t base,
                                            uint32_t rs, uint32_t re, uint32_t row_end,
                                            const double *s_prod, const uint32_t *s_col,
                                            double &acc, uint32_t row = 0) {
  if (MODE != MODE_CONSTRAINTS && SHORT) {
    // the sweep kernel's ranges (a row's elements inside one panel and tile) hold 0-2 elements
    // nearly always: two reads in flight instead of four halves the LDS instructions of its summing phase
    for (uint32_t i = rs; i < re; i += 2u) {
      const uint32_t k = i - base, last = re - 1u - base;
      const double a0 = s_prod[k], a1 = s_prod[min(k + 1u, last)];
      acc += a0;
      if (i + 1u < re) acc += a1;
    }
    return true;
  }
  if (MODE != MODE_CONSTRAINTS) {
    // four LDS reads in flight, then up to four adds in element order; a lane
    // past its row's end re-reads its last slot and skips the add (no "+ 0.0":
    // that could turn a -0.0 sum into +0.0)
    for (uint32_t i = rs; i < re; i += 4u) {
      const uint32_t k = i - base, last = re - 1u - base;
      const double a0 = s_prod[k], a1 = s_prod[min(k + 1u, last)], a2 = s_prod[min(k + 2u, last)],
                   a3 = s_prod[min(k + 3u, last)];
      acc += a0;
      if (i + 1u < re) acc += a1;
      if (i + 2u < re) acc += a2;
      if (i + 3u < re) acc += a3;
    }
    return true;
  }
  for (uint32_t i = rs; i < re; i++) {
    if (!csr_check_element(A, ev, base, i, re, row_end, s_col, row)) return false;
    acc += s_prod[i - base];
  }
  return true;
}

// CSR SpMV, all modes.  A workgroup owns a block of whole rows whose non-zeros
// fit one LDS tile (row blocks are cut at create time): phase 1 streams the
// block's cols/vals fully coalesced, checks ECC, gathers x and parks
// value*x in LDS; phase 2 gives each row to one thread, which adds its
// products in order.  A row longer than a tile is walked tile by tile with the
// running sum carried by thread 0 (same order, so still bit-exact).
//   reference: CSR/CPUContext.cpp:115-133 (none), :162-207 (constraints),
//              :214-245 (sed), :252-289 (sec7), :297-345 (sec8), :353-411 (secded)
// VECC (abft_hip_spmv_vecc): x and y hold protected elements.  Every gathered x and
// the fused product's x[row] get the full check (repaired in registers, reported, x itself not written
// back); y[row] is stored encoded and the fused product uses the decoded x[row] and the truncated sum.
// NUPD = 1 (cross-call fusion no. 4, abft_hip.hip "xpend"): the launch also applies the x += alpha p that the
// preceding calc_p left pending on the OLD p -- xu.xs[row] = xu.xs[row] + xu.u[0].alpha * xu.u[0].p_old[row] for every
// row of the workgroup's row block, exactly once, whatever becomes of the row (no elements, bad row
// pointers, a fatal element): two row-indexed, coalesced streams that hang off the block descriptor only
// and travel under the latency of the codes and the gathers.  Separate multiply and add
// (-ffp-contract=off): the bits axpy_kernel / calc_px_kernel give.  The row blocks partition
// [0, n_out) (cut_blocks), and the launch covers every block.
// NUPD = 2, 4 (no. 6, loop_state.h LazyUpdates): that many queued updates in one pass, oldest first -- x read once,
// NUPD old p's read beside it, xs = xs + a0 * p0; xs = xs + a1 * p1; ... and one store.  Exactly NUPD
// updates: a slot padded with alpha = 0 would turn -0.0 into +0.0 and 0 * inf into NaN.
#if ABFT_CFG_XUPD_NT  // the update's streams are touched once per launch: keep them out of the caches the gathers live in
#define XUPD_LOAD_P(p) ((ABFT_CFG_XUPD_NT & 1) ? __builtin_nontemporal_load(p) : *(p))
#define XUPD_LOAD_X(p) ((ABFT_CFG_XUPD_NT & 2) ? __builtin_nontemporal_load(p) : *(p))
#define XUPD_STORE_X(p, v) do { if (ABFT_CFG_XUPD_NT & 4) __builtin_nontemporal_store((v), (p)); else *(p) = (v); } while (0)
#else
#define XUPD_LOAD_P(p) (*(p))
#define XUPD_LOAD_X(p) (*(p))
#define XUPD_STORE_X(p, v) (*(p) = (v))
#endif
// the NUPD multiply-adds of one element, oldest first
// (scalars, not an array: the NUPD = 1 instantiation is instruction for instruction what it was before there were four)
template <int NUPD>
__device__ __forceinline__ void xupd_load(const XUpd &xu, uint32_t row, double &xs, double &po, double &po1, double &po2,
                                          double &po3) {
  xs = XUPD_LOAD_X(xu.xs + row);
  po = XUPD_LOAD_P(xu.u[0].p_old + row);
  if (NUPD > 1) po1 = XUPD_LOAD_P(xu.u[1].p_old + row);
  if (NUPD > 2) { po2 = XUPD_LOAD_P(xu.u[2].p_old + row); po3 = XUPD_LOAD_P(xu.u[3].p_old + row); }
}
template <int NUPD>
__device__ __forceinline__ double xupd_chain(const XUpd &xu, double xs, double po, double po1, double po2, double po3) {
  xs = xs + xu.u[0].alpha * po;
  if (NUPD > 1) xs = xs + xu.u[1].alpha * po1;
  if (NUPD > 2) { xs = xs + xu.u[2].alpha * po2; xs = xs + xu.u[3].alpha * po3; }
  return xs;
}
// what a matrix without fast records reads (CsrPackedFast): not packed, nothing proven.  In global memory like the
// records: picked against a __constant__ the address is a generic one, and the record comes through a flat load
// into vector registers.
__device__ uint4 k_no_record = {0u, 0u, 0u, 0u};
template <int MODE, int EPT, bool FUSE, bool VECC = false, int NUPD = 0>
__global__ __launch_bounds__(ABFT_BLOCK) void spmv_csr_kernel(CsrDev A, const double *__restrict__ x,
                                                              double *__restrict__ y, EventRing ev,
                                                              FuseOut fuse, TileSpan span, CsrCompact cc,
                                                              CsrPacked cp, XUpd xu, CsrPackedFast pf) {
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  constexpr bool FASTABLE = MODE == MODE_NONE && !VECC && ABFT_CFG_PACKED_PAL == 0;  // the instantiations that read pf (and not cp.pdesc)
  __shared__ __attribute__((aligned(16))) double s_prod[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[MODE == MODE_CONSTRAINTS ? TILE : 2];
  const uint32_t b = xcd_tile(blockIdx.x, span.count);
  const uint32_t t = span.first + b + (b >= span.cut ? span.skip : 0u);
  // mode none on plain vectors: the tile's record {packed-code descriptor, fast word} (CsrPackedFast; all 0: not
  // packed, nothing proven), uniform.  In front of the block descriptor on purpose: hipcc asks for a kernel argument
  // where it is first used, and with this one asked for behind `desc` the record's load waited for the descriptor's --
  // with the descriptor and the word loaded apart, as first built, three dependent round trips in front of every
  // workgroup's codes instead of one, which ate the path's whole gain (profiles/r15).
  // A matrix without records reads the one record of zeros below: the null test picks the address, not the value --
  // with the value picked behind a branch, the loaded record meets the zeros at a join and hipcc waits for it there.
  uint4 rec = make_uint4(0u, 0u, 0u, 0u);
  if (FASTABLE) rec = *(pf.rec ? pf.rec + t : &k_no_record);
  const uint4 desc = A.blk[t];  // one scalar load instead of two dependent pairs
  // mode none: this tile's column base (by tile, not workgroup: span cut / skip), uniform
  const uint32_t cb = (MODE == MODE_NONE && cc.cbase) ? cc.cbase[t] : ABFT_CBASE_WIDE;
  // ... and its packed-code descriptor (.y == 0: not packed), uniform as well
  const uint2 pd = FASTABLE ? make_uint2(rec.x, rec.y) : (MODE == MODE_NONE && cp.pdesc) ? cp.pdesc[t] : make_uint2(0u, 0u);
  const uint32_t fw = rec.z;
  // bit 31 of the second word: every row of this block has the same length (banded
  // matrices: nearly all blocks), so the row pointers need not be read at all
  const bool uniform = ABFT_CFG_UNIFORM_ROWS && MODE != MODE_CONSTRAINTS && (desc.y >> 31) != 0u;
  const uint32_t row0 = desc.x, row1 = desc.y & 0x7fffffffu, e0 = desc.z, e1 = desc.w;
  const uint32_t base = e0 & ~1u;
  double dsum = 0.0;  // FUSE: this thread's share of sum x[row] * y[row]

  if (FASTABLE && (fw >> ABFT_FAST_LEN_SHIFT) != 0u) {
    // one packed tile of at most ABFT_BLOCK rows of `len` elements each: nothing is tested per element or per row
    const uint32_t len = fw >> ABFT_FAST_LEN_SHIFT, row = row0 + threadIdx.x;
    const bool mine = row < row1;
    double xr = 0.0, xs = 0.0, po = 0.0, po1 = 0.0, po2 = 0.0, po3 = 0.0;
    if (FUSE && mine) xr = x[fuse.x_off + row];
    if (NUPD && mine) xupd_load<NUPD>(xu, row, xs, po, po1, po2, po3);
    csr_stage_packed_fast<EPT>(cp, pd, x, base, s_prod);
    __syncthreads();
    if (mine) {
      if (NUPD) XUPD_STORE_X(xu.xs + row, xupd_chain<NUPD>(xu, xs, po, po1, po2, po3));
      const double acc = csr_row_sum_len(s_prod + (e0 - base) + len * threadIdx.x, len);
      if (ABFT_CFG_Y_NT && NUPD) __builtin_nontemporal_store(acc, y + row);
      else y[row] = acc;
      if (FUSE) dsum += xr * acc;
    }
  } else if (e1 >= e0 && e1 - base <= TILE) {
    // row pointers for phase 2, requested before the tile so their latency overlaps
    const uint32_t r = row0 + threadIdx.x;
    uint32_t rs = 0, re = 0;
    double xr = 0.0;
    if (r < row1) {
      if (uniform) {
        const uint32_t len = (e1 - e0) / (row1 - row0);  // scalar
        rs = e0 + len * threadIdx.x; re = rs + len;
      } else {
        rs = A.rowptr[r]; re = A.rowptr[r + 1];
      }
      if (FUSE) xr = x[fuse.x_off + r];
    }
    double xs = 0.0, po = 0.0, po1 = 0.0, po2 = 0.0, po3 = 0.0;  // NUPD: the first row's operands, in flight beside the codes and the gathers
    if (NUPD && r < row1) xupd_load<NUPD>(xu, r, xs, po, po1, po2, po3);
    if (FASTABLE && fw != 0u)  // the stage bit alone: rows of several lengths, long ones, or more rows than threads
      csr_stage_packed_fast<EPT>(cp, pd, x, base, s_prod);
    else if (MODE == MODE_NONE && pd.y != 0u)
      csr_stage_packed<EPT, VECC>(A, cp, pd, x, ev, base, e0, e1, s_prod);
    else if (MODE == MODE_NONE)
      csr_stage_none<EPT, VECC>(A, cc, cb, x, ev, base, e0, e1, s_prod, s_col);
    else
      csr_stage<MODE, EPT, VECC>(A, x, ev, base, e0, e1, s_prod, s_col);
    __syncthreads();
    for (uint32_t row = r; row < row1; row += ABFT_BLOCK) {
      if (row != r) {
        rs = A.rowptr[row]; re = A.rowptr[row + 1];
        if (FUSE) xr = x[fuse.x_off + row];
        if (NUPD) xupd_load<NUPD>(xu, row, xs, po, po1, po2, po3);
      }
      if (NUPD) XUPD_STORE_X(xu.xs + row, xupd_chain<NUPD>(xu, xs, po, po1, po2, po3));  // in front of every `continue`: the update does not depend on the row
      if (MODE == MODE_CONSTRAINTS) {  // reference CSR/CPUContext.cpp:173-182
        if (re > A.nnz) { push_event(ev, ABFT_EV_ROW_SIZE, row, row, FMT_CSR); continue; }
        if (re < rs) { push_event(ev, ABFT_EV_ROW_ORDER, row, row, FMT_CSR); continue; }
      }
      if (rs < e0 || re > e1 || re < rs) continue;  // inconsistent row pointers: never touch LDS out of range
      double acc = 0.0;
      if (csr_row_sum<MODE>(A, ev, base, rs, re, re, s_prod, s_col, acc, row)) {
        if (VECC) {
          const uint64_t yw = vecc_encode(acc);
          y[row] = vecc_double(yw);
          if (FUSE) {
            uint64_t xw = vecc_bits(xr);
            if (__builtin_expect(vecc_suspect(xw) != 0u, 0)) xw = vecc_cold(xw, fuse.x_off + row, 0u, ev).w;
            dsum += vecc_value(xw) * vecc_value(yw);
          }
        } else {
          if (ABFT_CFG_Y_NT && NUPD && MODE == MODE_NONE) __builtin_nontemporal_store(acc, y + row);  // w ends at the boundary calc_r waits behind
          else y[row] = acc;
          if (FUSE) dsum += xr * acc;
        }
      }
    }
  } else {
    // long row (or inconsistent pointers): rows of this block one at a time, tile by tile
    if (NUPD)
      for (uint32_t row = row0 + threadIdx.x; row < row1; row += ABFT_BLOCK) {
        double xs = 0.0, po = 0.0, po1 = 0.0, po2 = 0.0, po3 = 0.0;
        xupd_load<NUPD>(xu, row, xs, po, po1, po2, po3);
        XUPD_STORE_X(xu.xs + row, xupd_chain<NUPD>(xu, xs, po, po1, po2, po3));
      }
    for (uint32_t row = row0; row < row1; row++) {
      const uint32_t rs = A.rowptr[row], re = A.rowptr[row + 1];
      if (MODE == MODE_CONSTRAINTS) {
        if (re > A.nnz) { if (threadIdx.x == 0) push_event(ev, ABFT_EV_ROW_SIZE, row, row, FMT_CSR); continue; }
        if (re < rs) { if (threadIdx.x == 0) push_event(ev, ABFT_EV_ROW_ORDER, row, row, FMT_CSR); continue; }
      }
      if (re > A.nnz || re < rs) continue;
      double acc = 0.0;
      bool ok = true;
      for (uint32_t lo = rs; lo < re;) {
        const uint32_t b = lo & ~1u;
        const uint32_t hi = min(re, b + TILE);
        __syncthreads();
        csr_stage<MODE, EPT, VECC>(A, x, ev, b, lo, hi, s_prod, s_col);
        __syncthreads();
        if (threadIdx.x == 0 && ok) ok = csr_row_sum<MODE>(A, ev, b, lo, hi, re, s_prod, s_col, acc, row);
        lo = hi;
      }
      if (threadIdx.x == 0 && ok) {
        if (VECC) {
          const uint64_t yw = vecc_encode(acc);
          y[row] = vecc_double(yw);
          if (FUSE) dsum += vecc_decode_cold_ok(x + fuse.x_off + row, fuse.x_off + row, 0u, ev) * vecc_value(yw);
        } else {
          y[row] = acc;
          if (FUSE) dsum += x[fuse.x_off + row] * acc;
        }
      }
    }
  }
  if (FUSE) fused_dot_finish(dsum, fuse, t);
}

// Panel-layout CSR SpMV (see CsrPanels).  Persistent workgroups: each takes row
// groups g, g + gridDim.x, ... and, per group, sweeps the column panels in
// ascending order with the 4 row sums of every thread held in registers.  A
// segment is staged through LDS by the same branch-free load phase as the
// streaming kernel (fully coalesced, ECC in registers); each thread then adds
// the staged products of its rows, in element order, onto its running sums.
template <int MODE, int EPT, bool FUSE>
__global__ __launch_bounds__(ABFT_BLOCK) void spmv_csr_panels_kernel(CsrDev A, CsrPanels P,
                                                                     const double *__restrict__ x,
                                                                     double *__restrict__ y, EventRing ev,
                                                                     FuseOut fuse, uint32_t c0, uint32_t c1) {
  // panels [c0, c1) in this launch; a launch that does not start at panel 0
  // resumes from the row sums the previous launch left in y (exact: fp64 stores)
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  constexpr int RPT = ABFT_PANEL_ROWS_PER_THREAD;
  __shared__ __attribute__((aligned(16))) double s_prod[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[2];
  double dsum = 0.0;
  for (uint32_t g = blockIdx.x; g < P.ngroups; g += gridDim.x) {
    const uint32_t row0 = g * ABFT_PANEL_ROWS;
    double acc[RPT];
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t row = row0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x;
      acc[j] = (c0 > 0 && row < A.n_out) ? y[row] : 0.0;
    }
    for (uint32_t c = c0; c < c1; c++) {
      const uint32_t seg = g * P.npanels + c;
      const uint32_t e0 = P.seg_base[seg], e1 = P.seg_base[seg + 1];
      if (e0 == e1) continue;  // uniform
      const uint16_t *ptr = P.seg_ptr + (size_t)seg * (ABFT_PANEL_ROWS + 1);
      uint32_t rs[RPT], re[RPT];
#pragma unroll
      for (int j = 0; j < RPT; j++) {  // this thread's rows: row0 + j*256 + tid
        const uint32_t r = (uint32_t)j * ABFT_BLOCK + threadIdx.x;
        rs[j] = e0 + ptr[r];
        re[j] = e0 + ptr[r + 1];
      }
      for (uint32_t lo = e0; lo < e1;) {
        const uint32_t b = lo & ~1u;
        const uint32_t hi = min(e1, b + TILE);
        __syncthreads();
        csr_stage<MODE, EPT>(A, x, ev, b, lo, hi, s_prod, s_col);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RPT; j++) {
          const uint32_t a0 = max(rs[j], lo), a1 = min(re[j], hi);
          if (a0 < a1) {
            double t = acc[j];
            csr_row_sum<MODE>(A, ev, b, a0, a1, a1, s_prod, s_col, t);
            acc[j] = t;
          }
        }
        lo = hi;
      }
    }
    double xo[FUSE ? RPT : 1];  // (the fused product's operands, in flight together)
    if (FUSE) {
#pragma unroll
      for (int j = 0; j < RPT; j++) xo[j] = x[fuse.x_off + min(row0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x, A.n_out - 1u)];
    }
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t row = row0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x;
      if (row < A.n_out) {
        y[row] = acc[j];
        if (FUSE) dsum += xo[j] * acc[j];
      }
    }
  }
  if (FUSE) fused_dot_finish(dsum, fuse, blockIdx.x);
}

template <int MODE>
static hipError_t launch_panels_mode(const CsrDev &A, const CsrPanels &P, const double *x, double *y,
                                     EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1,
                                     hipStream_t s) {
  if (fuse)
    hipLaunchKernelGGL((spmv_csr_panels_kernel<MODE, ABFT_CFG_PANEL_EPT, true>), dim3(grid), dim3(ABFT_BLOCK), 0,
                       s, A, P, x, y, ev, *fuse, c0, c1);
  else
    hipLaunchKernelGGL((spmv_csr_panels_kernel<MODE, ABFT_CFG_PANEL_EPT, false>), dim3(grid), dim3(ABFT_BLOCK), 0,
                       s, A, P, x, y, ev, FuseOut{}, c0, c1);
  return hipGetLastError();
}

// `chunk` panels per launch (0: all in one launch).  The kernel boundary between
// chunks is what keeps every workgroup of the chip in the same window of x; the
// fused dot rides on the last chunk only.
hipError_t launch_spmv_csr_panels(int mode, const CsrDev &A, const CsrPanels &P, const double *x, double *y,
                                  EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t chunk,
                                  hipStream_t s) {
  if (P.ngroups == 0) return hipSuccess;
  if (chunk == 0 || chunk > P.npanels) chunk = P.npanels;
  for (uint32_t c0 = 0; c0 < P.npanels; c0 += chunk) {
    const uint32_t c1 = c0 + chunk < P.npanels ? c0 + chunk : P.npanels;
    const FuseOut *f = c1 == P.npanels ? fuse : nullptr;
    hipError_t e;
    switch (mode) {
      case MODE_NONE: e = launch_panels_mode<MODE_NONE>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SED: e = launch_panels_mode<MODE_SED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC7: e = launch_panels_mode<MODE_SEC7>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC8: e = launch_panels_mode<MODE_SEC8>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SECDED: e = launch_panels_mode<MODE_SECDED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int MODE, bool FUSE> static int panels_occupancy() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spmv_csr_panels_kernel<MODE, ABFT_CFG_PANEL_EPT, FUSE>,
                                                   ABFT_BLOCK, 0) != hipSuccess || n < 1)
    n = 1;
  return n > 8 ? 8 : n;
}

int spmv_csr_panels_blocks_per_cu(int mode, bool fuse) {
  switch (mode) {
    case MODE_NONE: return fuse ? panels_occupancy<MODE_NONE, true>() : panels_occupancy<MODE_NONE, false>();
    case MODE_SED: return fuse ? panels_occupancy<MODE_SED, true>() : panels_occupancy<MODE_SED, false>();
    case MODE_SEC7: return fuse ? panels_occupancy<MODE_SEC7, true>() : panels_occupancy<MODE_SEC7, false>();
    case MODE_SEC8: return fuse ? panels_occupancy<MODE_SEC8, true>() : panels_occupancy<MODE_SEC8, false>();
    default: return fuse ? panels_occupancy<MODE_SECDED, true>() : panels_occupancy<MODE_SECDED, false>();
  }
}

template <int MODE>
static hipError_t launch_spmv_csr_mode(const CsrDev &A, const CsrCompact &cc, const CsrPacked &cp, const TileSpan &span,
                                       const double *x, double *y, EventRing ev, const FuseOut *fuse, hipStream_t s,
                                       bool vecc, const XUpd *xu, CsrPackedFast pf) {
  if (xu && xu->n == 4)
    hipLaunchKernelGGL((spmv_csr_kernel<MODE, ABFT_CSR_EPT, true, false, 4>), dim3(span.count), dim3(ABFT_BLOCK), 0,
                       s, A, x, y, ev, *fuse, span, cc, cp, *xu, pf);
  else if (xu && xu->n == 2)
    hipLaunchKernelGGL((spmv_csr_kernel<MODE, ABFT_CSR_EPT, true, false, 2>), dim3(span.count), dim3(ABFT_BLOCK), 0,
                       s, A, x, y, ev, *fuse, span, cc, cp, *xu, pf);
  else if (xu)
    hipLaunchKernelGGL((spmv_csr_kernel<MODE, ABFT_CSR_EPT, true, false, 1>), dim3(span.count), dim3(ABFT_BLOCK), 0,
                       s, A, x, y, ev, *fuse, span, cc, cp, *xu, pf);
  else if (vecc && fuse)
    hipLaunchKernelGGL((spmv_csr_kernel<MODE, ABFT_CSR_EPT, true, true>), dim3(span.count), dim3(ABFT_BLOCK), 0, s, A,
                       x, y, ev, *fuse, span, cc, cp, XUpd{}, pf);
  else if (vecc)
    hipLaunchKernelGGL((spmv_csr_kernel<MODE, ABFT_CSR_EPT, false, true>), dim3(span.count), dim3(ABFT_BLOCK), 0, s, A,
                       x, y, ev, FuseOut{}, span, cc, cp, XUpd{}, pf);
  else if (fuse) {
    hipLaunchKernelGGL((spmv_csr_kernel<MODE, ABFT_CSR_EPT, true>), dim3(span.count), dim3(ABFT_BLOCK), 0, s, A,
                       x, y, ev, *fuse, span, cc, cp, XUpd{}, pf);
  } else
    hipLaunchKernelGGL((spmv_csr_kernel<MODE, ABFT_CSR_EPT, false>), dim3(span.count), dim3(ABFT_BLOCK), 0, s, A,
                       x, y, ev, FuseOut{}, span, cc, cp, XUpd{}, pf);
  return hipGetLastError();
}

hipError_t launch_spmv_csr(int mode, const CsrDev &A, const CsrCompact &cc, const CsrPacked &cp, const TileSpan &span,
                           const double *x, double *y, EventRing ev, const FuseOut *fuse, hipStream_t s, bool vecc,
                           const XUpd *xu, CsrPackedFast pf) {
  // the x update rides on a launch of every row block with the fused product, plain vectors (abft_hip.hip decides)
  if (xu) {
    if (!fuse || vecc || span.first || span.skip || span.count != A.nblk || !span.count || !xu->xs) return hipErrorInvalidValue;
    if (xu->n != 1 && xu->n != 2 && xu->n != 4) return hipErrorInvalidValue;
    for (int k = 0; k < xu->n; k++)
      if (!xu->u[k].p_old) return hipErrorInvalidValue;
  }
  // every tile the span maps to must exist: checked here, on the host
  if (span.count == 0) return hipSuccess;
  if ((uint64_t)span.first + span.count + span.skip > A.nblk || span.cut > span.count) return hipErrorInvalidValue;
  // compact columns only in mode none, and then both arrays
  if ((cc.cbase || cc.cols16) && (mode != MODE_NONE || !cc.cbase || !cc.cols16)) return hipErrorInvalidValue;
  // packed codes likewise, and then all three arrays
  if ((cp.code16 || cp.pdesc || cp.pal) && (mode != MODE_NONE || !cp.code16 || !cp.pdesc || !cp.pal))
    return hipErrorInvalidValue;
  // the records come with the packed blocks, always: on plain vectors the kernel reads them in the descriptors' stead
  if ((pf.rec != nullptr) != (cp.pdesc != nullptr)) return hipErrorInvalidValue;
  switch (mode) {
    case MODE_NONE: return launch_spmv_csr_mode<MODE_NONE>(A, cc, cp, span, x, y, ev, fuse, s, vecc, xu, pf);
    case MODE_CONSTRAINTS: return launch_spmv_csr_mode<MODE_CONSTRAINTS>(A, cc, cp, span, x, y, ev, fuse, s, vecc, xu, pf);
    case MODE_SED: return launch_spmv_csr_mode<MODE_SED>(A, cc, cp, span, x, y, ev, fuse, s, vecc, xu, pf);
    case MODE_SEC7: return launch_spmv_csr_mode<MODE_SEC7>(A, cc, cp, span, x, y, ev, fuse, s, vecc, xu, pf);
    case MODE_SEC8: return launch_spmv_csr_mode<MODE_SEC8>(A, cc, cp, span, x, y, ev, fuse, s, vecc, xu, pf);
    case MODE_SECDED: return launch_spmv_csr_mode<MODE_SECDED>(A, cc, cp, span, x, y, ev, fuse, s, vecc, xu, pf);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------- protected row structure --
// The streaming kernel on a structure-protected matrix (struct_ecc.h): no plain row pointers and
// no plain descriptors exist.  A sibling of spmv_csr_kernel, not a further flag of it, so that none of its
// instantiations moves; csr_stage, csr_row_sum, fused_dot_finish and the vector-ECC pieces are shared.  Such a matrix
// has neither compact nor packed blocks and is never a partner of the x-update fusions.
//
// Cold paths, out of line.  Every stored word has ONE owner per launch -- a row word the lane that sums the row
// (thread 0 in the long-row branch, where all threads read it), a descriptor thread 0 of its workgroup --, and only the
// owner stores the repaired word back (a plain vector store) and queues the event.
__device__ __noinline__ VeccWord rowext_cold(uint64_t word, uint64_t *at, uint32_t row, bool owner, EventRing ev) {
  VeccWord o;
  uint32_t bit;
  vecc_repair(word, o, bit);
  if (owner && o.rc) {
    if (o.rc > 0) *at = o.w;
    push_event(ev, o.rc > 0 ? ABFT_EV_STRUCT_CORRECTED : ABFT_EV_STRUCT_DOUBLE, row, bit | (ABFT_STRUCT_ROW << 8), ABFT_FMT_CSR);
  }
  return o;
}

__device__ __noinline__ StructBlk blk_cold(uint4 d, uint4 *at, uint32_t t, bool owner, EventRing ev) {
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  StructBlk o;
  uint32_t bit;
  blk_repair(w, o, bit);
  if (owner && o.rc) {
    if (o.rc > 0) *at = make_uint4(o.w[0], o.w[1], o.w[2], o.w[3]);
    push_event(ev, o.rc > 0 ? ABFT_EV_STRUCT_CORRECTED : ABFT_EV_STRUCT_DOUBLE, t, (o.rc > 0 ? bit : 0u) | (ABFT_STRUCT_BLOCK << 8),
               ABFT_FMT_CSR);
  }
  return o;
}

template <int MODE, int EPT, bool FUSE, bool VECC>
__global__ __launch_bounds__(ABFT_BLOCK) void spmv_csr_struct_kernel(CsrDev A, CsrStruct S, const double *__restrict__ x,
                                                                     double *__restrict__ y, EventRing ev, FuseOut fuse,
                                                                     TileSpan span) {
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  __shared__ __attribute__((aligned(16))) double s_prod[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[MODE == MODE_CONSTRAINTS ? TILE : 2];
  const uint32_t b = xcd_tile(blockIdx.x, span.count);
  const uint32_t t = span.first + b + (b >= span.cut ? span.skip : 0u);
  uint4 desc = S.blk[t];  // uniform, 16 bytes, as in spmv_csr_kernel
  bool dead = false;      // two flips in the descriptor: nothing derived from it is used (uniform)
  {
    const uint32_t w[4] = {desc.x, desc.y, desc.z, desc.w};
    if (__builtin_expect(blk_suspect(w) != 0u, 0)) {
      const StructBlk o = blk_cold(desc, S.blk + t, t, threadIdx.x == 0, ev);
      dead = o.rc < 0;
      desc = make_uint4(o.w[0], o.w[1], o.w[2], o.w[3]);
    }
  }
  const bool uniform = ABFT_CFG_UNIFORM_ROWS && MODE != MODE_CONSTRAINTS && (desc.y >> 31) != 0u;
  // (a descriptor that passed its check holds what create stored; the clamps cost two scalar instructions and keep a
  // mis-decoded word of three or more flips inside the arrays)
  const uint32_t row1 = min(desc.y & 0x7fffffffu, A.n_out), row0 = min(blk_first_row(desc.x), row1);
  const uint32_t e1 = min(desc.w, A.nnz), e0 = desc.z;
  const uint32_t base = e0 & ~1u;
  double dsum = 0.0;  // FUSE: this thread's share of sum x[row] * y[row]; a dead workgroup leaves a zero partial

  if (dead) {
  } else if (e1 >= e0 && e1 - base <= TILE) {
    // the first row's word for phase 2, requested before the tile so its latency overlaps
    const uint32_t r = row0 + threadIdx.x;
    uint32_t rs = 0, re = 0;
    uint64_t rw = 0;
    double xr = 0.0;
    if (r < row1) {
      if (uniform) {
        const uint32_t len = (e1 - e0) / (row1 - row0);  // scalar: from the checked descriptor, no row word is read
        rs = e0 + len * threadIdx.x; re = rs + len;
      } else {
        rw = S.rowext[r];
      }
      if (FUSE) xr = x[fuse.x_off + r];
    }
    csr_stage<MODE, EPT, VECC>(A, x, ev, base, e0, e1, s_prod, s_col);
    __syncthreads();
    for (uint32_t row = r; row < row1; row += ABFT_BLOCK) {
      if (row != r) {
        rw = S.rowext[row];
        if (FUSE) xr = x[fuse.x_off + row];
      }
      if (!uniform || row != r) {
        if (__builtin_expect(vecc_suspect(rw) != 0u, 0)) {
          const VeccWord o = rowext_cold(rw, S.rowext + row, row, true, ev);
          if (o.rc < 0) continue;  // two flips: y[row] is not written
          rw = o.w;
        }
        rs = rowext_start(rw); re = rowext_end(rw);
      }
      if (MODE == MODE_CONSTRAINTS) {  // reference CSR/CPUContext.cpp:173-182
        if (re > A.nnz) { push_event(ev, ABFT_EV_ROW_SIZE, row, row, FMT_CSR); continue; }
        if (re < rs) { push_event(ev, ABFT_EV_ROW_ORDER, row, row, FMT_CSR); continue; }
      }
      if (rs < e0 || re > e1 || re < rs) continue;  // inconsistent extents: never touch LDS out of range
      double acc = 0.0;
      if (csr_row_sum<MODE>(A, ev, base, rs, re, re, s_prod, s_col, acc, row)) {
        if (VECC) {
          const uint64_t yw = vecc_encode(acc);
          y[row] = vecc_double(yw);
          if (FUSE) {
            uint64_t xw = vecc_bits(xr);
            if (__builtin_expect(vecc_suspect(xw) != 0u, 0)) xw = vecc_cold(xw, fuse.x_off + row, 0u, ev).w;
            dsum += vecc_value(xw) * vecc_value(yw);
          }
        } else {
          y[row] = acc;
          if (FUSE) dsum += xr * acc;
        }
      }
    }
  } else {
    // long row (or inconsistent element bounds): rows of this block one at a time, tile by tile.  Every thread reads
    // the row's word, uniformly; thread 0 alone reports and stores back.
    for (uint32_t row = row0; row < row1; row++) {
      uint64_t rw = S.rowext[row];
      if (__builtin_expect(vecc_suspect(rw) != 0u, 0)) {
        const VeccWord o = rowext_cold(rw, S.rowext + row, row, threadIdx.x == 0, ev);
        if (o.rc < 0) continue;
        rw = o.w;
      }
      const uint32_t rs = rowext_start(rw), re = rowext_end(rw);
      if (MODE == MODE_CONSTRAINTS) {
        if (re > A.nnz) { if (threadIdx.x == 0) push_event(ev, ABFT_EV_ROW_SIZE, row, row, FMT_CSR); continue; }
        if (re < rs) { if (threadIdx.x == 0) push_event(ev, ABFT_EV_ROW_ORDER, row, row, FMT_CSR); continue; }
      }
      if (re > A.nnz || re < rs) continue;
      double acc = 0.0;
      bool ok = true;
      for (uint32_t lo = rs; lo < re;) {
        const uint32_t b = lo & ~1u;
        const uint32_t hi = min(re, b + TILE);
        __syncthreads();
        csr_stage<MODE, EPT, VECC>(A, x, ev, b, lo, hi, s_prod, s_col);
        __syncthreads();
        if (threadIdx.x == 0 && ok) ok = csr_row_sum<MODE>(A, ev, b, lo, hi, re, s_prod, s_col, acc, row);
        lo = hi;
      }
      if (threadIdx.x == 0 && ok) {
        if (VECC) {
          const uint64_t yw = vecc_encode(acc);
          y[row] = vecc_double(yw);
          if (FUSE) dsum += vecc_decode_cold_ok(x + fuse.x_off + row, fuse.x_off + row, 0u, ev) * vecc_value(yw);
        } else {
          y[row] = acc;
          if (FUSE) dsum += x[fuse.x_off + row] * acc;
        }
      }
    }
  }
  if (FUSE) fused_dot_finish(dsum, fuse, t);
}

template <int MODE>
static hipError_t launch_spmv_csr_struct_mode(const CsrDev &A, const CsrStruct &S, const TileSpan &span, const double *x,
                                              double *y, EventRing ev, const FuseOut *fuse, hipStream_t s, bool vecc) {
  const dim3 grid(span.count), block(ABFT_BLOCK);
  if (vecc && fuse)
    hipLaunchKernelGGL((spmv_csr_struct_kernel<MODE, ABFT_CSR_EPT, true, true>), grid, block, 0, s, A, S, x, y, ev, *fuse, span);
  else if (vecc)
    hipLaunchKernelGGL((spmv_csr_struct_kernel<MODE, ABFT_CSR_EPT, false, true>), grid, block, 0, s, A, S, x, y, ev, FuseOut{}, span);
  else if (fuse)
    hipLaunchKernelGGL((spmv_csr_struct_kernel<MODE, ABFT_CSR_EPT, true, false>), grid, block, 0, s, A, S, x, y, ev, *fuse, span);
  else
    hipLaunchKernelGGL((spmv_csr_struct_kernel<MODE, ABFT_CSR_EPT, false, false>), grid, block, 0, s, A, S, x, y, ev, FuseOut{}, span);
  return hipGetLastError();
}

hipError_t launch_spmv_csr_struct(int mode, const CsrDev &A, const CsrStruct &S, const TileSpan &span, const double *x,
                                  double *y, EventRing ev, const FuseOut *fuse, hipStream_t s, bool vecc) {
  if (!S.rowext || !S.blk) return hipErrorInvalidValue;
  // every tile the span maps to must exist: checked here, on the host
  if (span.count == 0) return hipSuccess;
  if ((uint64_t)span.first + span.count + span.skip > A.nblk || span.cut > span.count) return hipErrorInvalidValue;
  switch (mode) {
    case MODE_NONE: return launch_spmv_csr_struct_mode<MODE_NONE>(A, S, span, x, y, ev, fuse, s, vecc);
    case MODE_CONSTRAINTS: return launch_spmv_csr_struct_mode<MODE_CONSTRAINTS>(A, S, span, x, y, ev, fuse, s, vecc);
    case MODE_SED: return launch_spmv_csr_struct_mode<MODE_SED>(A, S, span, x, y, ev, fuse, s, vecc);
    case MODE_SEC7: return launch_spmv_csr_struct_mode<MODE_SEC7>(A, S, span, x, y, ev, fuse, s, vecc);
    case MODE_SEC8: return launch_spmv_csr_struct_mode<MODE_SEC8>(A, S, span, x, y, ev, fuse, s, vecc);
    case MODE_SECDED: return launch_spmv_csr_struct_mode<MODE_SECDED>(A, S, span, x, y, ev, fuse, s, vecc);
    default: return hipErrorInvalidValue;
  }
}

// create: the packed row words and the plain descriptors, as uploaded, get their codes in place
__global__ __launch_bounds__(ABFT_BLOCK) void struct_encode_kernel(CsrStruct S, uint32_t n, uint32_t nblk) {
  const uint32_t stride = gridDim.x * ABFT_BLOCK;
  for (uint32_t i = blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) S.rowext[i] = rowext_code(S.rowext[i]);
  for (uint32_t i = blockIdx.x * ABFT_BLOCK + threadIdx.x; i < nblk; i += stride) {
    const uint4 d = S.blk[i];
    uint32_t w[4] = {d.x, d.y, d.z, d.w};
    blk_encode(w);
    S.blk[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// Scrub: every row word and every descriptor -- the row words of uniform blocks too, which no SpMV reads --, one
// thread each: single flips repaired in place and reported like the SpMV does, counts[0] += repaired words,
// counts[1] += uncorrectable ones.
__global__ __launch_bounds__(ABFT_BLOCK) void struct_scrub_kernel(CsrStruct S, uint32_t n, uint32_t nblk, uint32_t *counts,
                                                                  EventRing ev) {
  const uint32_t stride = gridDim.x * ABFT_BLOCK;
  for (uint32_t i = blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    const uint64_t w = S.rowext[i];
    if (__builtin_expect(vecc_suspect(w) != 0u, 0)) {
      const VeccWord o = rowext_cold(w, S.rowext + i, i, true, ev);
      if (o.rc) atomicAdd(counts + (o.rc > 0 ? 0 : 1), 1u);
    }
  }
  for (uint32_t i = blockIdx.x * ABFT_BLOCK + threadIdx.x; i < nblk; i += stride) {
    const uint4 d = S.blk[i];
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
    if (__builtin_expect(blk_suspect(w) != 0u, 0)) {
      const StructBlk o = blk_cold(d, S.blk + i, i, true, ev);
      if (o.rc) atomicAdd(counts + (o.rc > 0 ? 0 : 1), 1u);
    }
  }
}

static uint32_t struct_grid(uint32_t n, uint32_t nblk) {
  const uint32_t most = n > nblk ? n : nblk;
  const uint32_t nb = (most + ABFT_BLOCK - 1) / ABFT_BLOCK;
  return nb < 1u ? 1u : nb > 4096u ? 4096u : nb;
}

hipError_t launch_struct_encode(const CsrStruct &S, uint32_t n, uint32_t nblk, hipStream_t s) {
  hipLaunchKernelGGL(struct_encode_kernel, dim3(struct_grid(n, nblk)), dim3(ABFT_BLOCK), 0, s, S, n, nblk);
  return hipGetLastError();
}

hipError_t launch_struct_scrub(const CsrStruct &S, uint32_t n, uint32_t nblk, uint32_t *counts, EventRing ev, hipStream_t s) {
  hipLaunchKernelGGL(struct_scrub_kernel, dim3(struct_grid(n, nblk)), dim3(ABFT_BLOCK), 0, s, S, n, nblk, counts, ev);
  return hipGetLastError();
}

// ------------------------------------------------------- CSR block SpMV (SpMM) --
// Y = A X for K right-hand sides at once (2 <= K <= 8; K = 1 is abft_hip_spmv).  A block
// vector is row-major: entry (i, j) at i*K + j, so the K entries a matrix element multiplies
// sit in one 8K-byte run.  Same row blocks and the same branch-free coalesced load phase
// (csr_issue_loads) as spmv_csr_kernel, so every element is loaded and ECC-checked ONCE per
// pass whatever K is; what goes to LDS is the CHECKED element -- its value and column, 12 B --
// not K products (TILE * K doubles would be 64 KB at K = 8).  Phase 2 gives each row to one
// thread, which gathers the K-wide rows of X (16-byte loads) and keeps K running sums, each
// added in ascending element order with separate multiply and add: column j of Y is the
// bits abft_hip_spmv gives for column j of X.  The cases spmv_csr_kernel stages a special
// product for, staged here so that value * x is that product for every column:
//   element outside the tile range  -> never summed (the rows' ranges exclude it)
//   fatal element (given up)        -> value +0.0, column ~0u: +0.0 * 0.0 = +0.0, as staged there
//   column >= n_in (mode none)      -> x taken as 0.0: value * 0.0, as there
#define SPMM_NO_COL 0xffffffffu

// ECC check of a tile whose loads were issued into `t`; the checked elements -> LDS.
// The cold path (repair + write-back, or give up) runs once per element per pass.
template <int MODE, int EPT>
__device__ __forceinline__ void spmm_stage(const CsrDev &A, const EventRing &ev, uint32_t base, uint32_t lo,
                                           uint32_t hi, double *s_val, uint32_t *s_col) {
  constexpr int STEPS = EPT / 2;
  CsrTileRegs<EPT> t;
  csr_issue_loads<EPT>(A, base, hi, t);
  uint32_t col[EPT];
  double val[EPT];
  uint32_t bad = 0u;
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const int s = j >> 1;
    const uint32_t i = base + 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK) + (uint32_t)(j & 1);
    const double d = (j & 1) ? t.v[s].y : t.v[s].x;
    uint32_t w[3] = {(uint32_t)__double2loint(d), (uint32_t)__double2hiint(d), (j & 1) ? t.c[s].y : t.c[s].x};
    const bool valid = i >= lo && i < hi;
    if (MODE >= MODE_SED) {
      if (valid && ecc_suspect<FMT_CSR, MODE>(w) != 0) bad |= 1u << j;
      w[2] &= ABFT_COLMASK;  // reference CSR/CPUContext.cpp:238, 282, 338, 404
    }
    col[j] = valid ? w[2] : SPMM_NO_COL;
    val[j] = valid ? as_double(w[0], w[1]) : 0.0;
  }
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const uint32_t k = 2u * threadIdx.x + (uint32_t)s * (2u * ABFT_BLOCK);
    *reinterpret_cast<double2 *>(s_val + k) = make_double2(val[2 * s], val[2 * s + 1]);
    *reinterpret_cast<uint2 *>(s_col + k) = make_uint2(col[2 * s], col[2 * s + 1]);
  }
  if (MODE >= MODE_SED && __builtin_expect(bad != 0u, 0)) {
    // as in csr_consume: the noted elements again, from memory, through the cold path
#pragma unroll 1
    for (uint32_t j = 0; j < (uint32_t)EPT; j++) {
      if (!((bad >> j) & 1u)) continue;
      const uint32_t i = base + 2u * threadIdx.x + (j >> 1) * (2u * ABFT_BLOCK) + (j & 1u);
      const double d = A.vals[i];
      EccWords<FMT_CSR> e;
      e.w[0] = (uint32_t)__double2loint(d); e.w[1] = (uint32_t)__double2hiint(d); e.w[2] = A.cols[i]; e.rc = 0;
      e = ecc_cold<FMT_CSR, MODE>(e, event_index(A, i), ev);
      double v = 0.0;
      uint32_t c = SPMM_NO_COL;
      if (e.rc > 0) {
        A.vals[i] = as_double(e.w[0], e.w[1]);
        A.cols[i] = e.w[2];
        v = as_double(e.w[0], e.w[1]);
        c = e.w[2] & ABFT_COLMASK;
      }
      s_val[i - base] = v;
      s_col[i - base] = c;
    }
  }
}

// the K entries of row c of a block vector (0.0 for a column past the vector: x taken as 0)
template <int K>
__device__ __forceinline__ void spmm_gather(const double *__restrict__ x, uint32_t c, uint32_t n_in, double *xv) {
  const bool in = c < n_in;  // a corrupted index must never fault the GPU
  const double *p = x + (size_t)(in ? c : 0u) * K;
  if (K % 2 == 0) {
#pragma unroll
    for (int j = 0; j < K; j += 2) {
      const double2 v = *reinterpret_cast<const double2 *>(p + j);
      xv[j] = in ? v.x : 0.0;
      xv[j + 1] = in ? v.y : 0.0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; j++) xv[j] = in ? p[j] : 0.0;
  }
}

// VECC (abft_hip_spmm_dot_vecc): the gathered rows of x are codewords.  In the gather/add
// loops a word is decoded to its value and one that fails vecc_suspect is only NOTED (no call where loads are in
// flight) ...
template <int K>
__device__ __forceinline__ uint32_t spmm_decode(double *xv) {
  uint32_t sus = 0u;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const uint64_t w = vecc_bits(xv[j]);
    sus |= vecc_suspect(w);
    xv[j] = vecc_value(w);
  }
  return sus;
}

// ... and a row (in the long-row path: the current tile's share of it) whose gathers held a noted word is summed a
// second time here, from the sums it started with, one element at a time: every word through the full decode
// (repaired in registers, reported once; x is not written back -- many rows gather the same entry, and calc_px
// rewrites it next).  Same elements, same order of adds: the sums have the undamaged call's bits.
template <int K>
__device__ __forceinline__ void spmm_row_redo(const double *__restrict__ x, uint32_t n_in, uint32_t k0, uint32_t k1,
                                              const double *s_val, const uint32_t *s_col, EventRing ev, double *acc) {
#pragma unroll 1
  for (uint32_t k = k0; k < k1; k++) {
    const uint32_t c = s_col[k];
    const double v = s_val[k];
    const bool in = c < n_in;
    const uint32_t at = (in ? c : 0u) * (uint32_t)K;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const double xj = in ? vecc_decode_cold_ok(x + at + j, at + (uint32_t)j, 0u, ev) : 0.0;
      acc[j] += v * xj;
    }
  }
}

// Row sums of elements [rs, re) from the staged elements, K columns, ascending element order.
// Constraints mode runs csr_row_sum's checks (csr_check_element) in the same order, so the
// same events are queued; returns false if a fatal one was.
template <int MODE, int K, bool VECC = false>
__device__ __forceinline__ bool spmm_row_sum(const CsrDev &A, const EventRing &ev, const double *__restrict__ x,
                                             uint32_t base, uint32_t rs, uint32_t re, uint32_t row_end,
                                             const double *s_val, const uint32_t *s_col, double *acc,
                                             uint32_t row) {
  double start[K];  // VECC: the sums the row came in with, for the second summation
  uint32_t sus = 0u;
  if (VECC) {
#pragma unroll
    for (int j = 0; j < K; j++) start[j] = acc[j];
  }
  if (MODE == MODE_CONSTRAINTS) {
    for (uint32_t i = rs; i < re; i++) {
      if (!csr_check_element(A, ev, base, i, re, row_end, s_col, row)) return false;
      double xv[K];
      spmm_gather<K>(x, s_col[i - base], A.n_in, xv);
      if (VECC) sus |= spmm_decode<K>(xv);
      const double v = s_val[i - base];
#pragma unroll
      for (int j = 0; j < K; j++) acc[j] += v * xv[j];
    }
    if (VECC && __builtin_expect(sus != 0u, 0)) {  // (every element passed its checks above: they are not run again)
#pragma unroll
      for (int j = 0; j < K; j++) acc[j] = start[j];
      spmm_row_redo<K>(x, A.n_in, rs - base, re - base, s_val, s_col, ev, acc);
    }
    return true;
  }
  // U elements' gathers in flight, then their adds in element order; a lane past its row's end
  // re-reads its last slot and skips the add (no "+ 0.0": that could turn a -0.0 sum into +0.0)
  constexpr int U = K <= 4 ? 4 : 2;
  for (uint32_t i = rs; i < re; i += U) {
    const uint32_t k = i - base, last = re - 1u - base;
    double v[U], xv[U][K];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t ku = min(k + (uint32_t)u, last);
      v[u] = s_val[ku];
      spmm_gather<K>(x, s_col[ku], A.n_in, xv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (VECC) sus |= spmm_decode<K>(xv[u]);
      if (u == 0 || i + (uint32_t)u < re) {
#pragma unroll
        for (int j = 0; j < K; j++) acc[j] += v[u] * xv[u][j];
      }
    }
  }
  if (VECC && __builtin_expect(sus != 0u, 0)) {
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = start[j];
    spmm_row_redo<K>(x, A.n_in, rs - base, re - base, s_val, s_col, ev, acc);
  }
  return true;
}

template <int K>
__device__ __forceinline__ void spmm_store_row(double *__restrict__ y, uint32_t row, const double *acc) {
  double *p = y + (size_t)row * K;
  if (K % 2 == 0) {
#pragma unroll
    for (int j = 0; j < K; j += 2) *reinterpret_cast<double2 *>(p + j) = make_double2(acc[j], acc[j + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < K; j++) p[j] = acc[j];
  }
}

// this thread's share of the K column products: dsum[j] += x[row, j] * y[row, j], y's row in registers
// (separate multiply and add; the row of x by the gathers' 16-byte loads)
template <int K>
__device__ __forceinline__ void spmm_dot_row(const double *__restrict__ x, uint32_t row, uint32_t n_in,
                                             const double *acc, double *dsum) {
  double xr[K];
  spmm_gather<K>(x, row, n_in, xr);
#pragma unroll
  for (int j = 0; j < K; j++) dsum[j] += xr[j] * acc[j];
}

// VECC: row `row` of y stored encoded, and this thread's share of the K products from the decoded x[row, j] and
// the stored word without its code bits (spmv_vecc's rule); x's row through the same two steps as the gathers:
// checked, and only a row with a suspect word goes through the full decode
template <int K>
__device__ __forceinline__ void spmm_finish_row_vecc(const double *__restrict__ x, double *__restrict__ y, uint32_t row,
                                                     uint32_t n_in, const EventRing &ev, double *acc, double *dsum) {
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = vecc_double(vecc_encode(acc[j]));
  spmm_store_row<K>(y, row, acc);
  double xr[K];
  spmm_gather<K>(x, row, n_in, xr);
  if (__builtin_expect(spmm_decode<K>(xr) != 0u, 0)) {
    const uint32_t at = row * (uint32_t)K;
#pragma unroll
    for (int j = 0; j < K; j++) xr[j] = vecc_decode_cold_ok(x + at + j, at + (uint32_t)j, 0u, ev);
  }
#pragma unroll
  for (int j = 0; j < K; j++) dsum[j] += xr[j] * vecc_value(vecc_bits(acc[j]));
}

// The block form of spmv_csr_kernel, whole matrix (reference lines as there).
// DOT (abft_hip_spmm_dot): a square matrix; the thread that stores y[row, 0..K)
// also adds x[row, j] * y[row, j] to its K running products -- a row of a long-row block once, when
// thread 0's carried sums are complete.  The workgroup leaves K partials (block_sum's shape per column),
// column j's at dotp[j * A.nblk + tile], with plain stores and exits, as fused_dot_finish does: no ticket
// here.  spmm_fold_kernel, launched behind, folds them in a fixed order.
// VECC (with DOT only; abft_hip_spmm_dot_vecc): x and y hold protected elements -- spmm_row_sum and
// spmm_finish_row_vecc above.
template <int MODE, int EPT, int K, bool DOT = false, bool VECC = false>
__global__ __launch_bounds__(ABFT_BLOCK) void spmm_csr_kernel(CsrDev A, const double *__restrict__ x,
                                                              double *__restrict__ y, EventRing ev,
                                                              double *__restrict__ dotp) {
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  __shared__ __attribute__((aligned(16))) double s_val[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[TILE];
  double dsum[K];
  if (DOT) {
#pragma unroll
    for (int j = 0; j < K; j++) dsum[j] = 0.0;
  }
  const uint32_t t = xcd_tile(blockIdx.x, A.nblk);
  const uint4 desc = A.blk[t];
  const bool uniform = ABFT_CFG_UNIFORM_ROWS && MODE != MODE_CONSTRAINTS && (desc.y >> 31) != 0u;
  const uint32_t row0 = desc.x, row1 = desc.y & 0x7fffffffu, e0 = desc.z, e1 = desc.w;
  const uint32_t base = e0 & ~1u;

  if (e1 >= e0 && e1 - base <= TILE) {
    const uint32_t r = row0 + threadIdx.x;
    uint32_t rs = 0, re = 0;
    if (r < row1) {
      if (uniform) {
        const uint32_t len = (e1 - e0) / (row1 - row0);
        rs = e0 + len * threadIdx.x; re = rs + len;
      } else {
        rs = A.rowptr[r]; re = A.rowptr[r + 1];
      }
    }
    spmm_stage<MODE, EPT>(A, ev, base, e0, e1, s_val, s_col);
    __syncthreads();
    for (uint32_t row = r; row < row1; row += ABFT_BLOCK) {
      if (row != r) { rs = A.rowptr[row]; re = A.rowptr[row + 1]; }
      if (MODE == MODE_CONSTRAINTS) {  // reference CSR/CPUContext.cpp:173-182
        if (re > A.nnz) { push_event(ev, ABFT_EV_ROW_SIZE, row, row, FMT_CSR); continue; }
        if (re < rs) { push_event(ev, ABFT_EV_ROW_ORDER, row, row, FMT_CSR); continue; }
      }
      if (rs < e0 || re > e1 || re < rs) continue;  // inconsistent row pointers: never touch LDS out of range
      double acc[K];
#pragma unroll
      for (int j = 0; j < K; j++) acc[j] = 0.0;
      if (spmm_row_sum<MODE, K, VECC>(A, ev, x, base, rs, re, re, s_val, s_col, acc, row)) {
        if (VECC) {
          spmm_finish_row_vecc<K>(x, y, row, A.n_in, ev, acc, dsum);
        } else {
          spmm_store_row<K>(y, row, acc);
          if (DOT) spmm_dot_row<K>(x, row, A.n_in, acc, dsum);
        }
      }
    }
  } else {
    // long row (or inconsistent pointers): rows of this block one at a time, tile by tile, the K
    // running sums carried by thread 0
    for (uint32_t row = row0; row < row1; row++) {
      const uint32_t rs = A.rowptr[row], re = A.rowptr[row + 1];
      if (MODE == MODE_CONSTRAINTS) {
        if (re > A.nnz) { if (threadIdx.x == 0) push_event(ev, ABFT_EV_ROW_SIZE, row, row, FMT_CSR); continue; }
        if (re < rs) { if (threadIdx.x == 0) push_event(ev, ABFT_EV_ROW_ORDER, row, row, FMT_CSR); continue; }
      }
      if (re > A.nnz || re < rs) continue;
      double acc[K];
#pragma unroll
      for (int j = 0; j < K; j++) acc[j] = 0.0;
      bool ok = true;
      for (uint32_t lo = rs; lo < re;) {
        const uint32_t b = lo & ~1u;
        const uint32_t hi = min(re, b + TILE);
        __syncthreads();
        spmm_stage<MODE, EPT>(A, ev, b, lo, hi, s_val, s_col);
        __syncthreads();
        if (threadIdx.x == 0 && ok) ok = spmm_row_sum<MODE, K, VECC>(A, ev, x, b, lo, hi, re, s_val, s_col, acc, row);
        lo = hi;
      }
      if (threadIdx.x == 0 && ok) {
        if (VECC) {
          spmm_finish_row_vecc<K>(x, y, row, A.n_in, ev, acc, dsum);
        } else {
          spmm_store_row<K>(y, row, acc);
          if (DOT) spmm_dot_row<K>(x, row, A.n_in, acc, dsum);
        }
      }
    }
  }
  if (DOT) {
    __shared__ double s_w[4 * K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const double bsum = block_sum(dsum[j], s_w + 4 * j);
      if (threadIdx.x == 0) dotp[(size_t)j * A.nblk + t] = bsum;
    }
  }
}

template <int MODE, bool DOT, bool VECC = false>
static hipError_t launch_spmm_csr_mode(int k, const CsrDev &A, const double *x, double *y, EventRing ev,
                                       double *dotp, hipStream_t s) {
  const dim3 g(A.nblk), b(ABFT_BLOCK);
#define ABFT_OP(K) hipLaunchKernelGGL((spmm_csr_kernel<MODE, ABFT_CSR_EPT, K, DOT, VECC>), g, b, 0, s, A, x, y, ev, dotp)
  switch (k) {
    case 1:  // without DOT, k = 1 is launch_spmv_csr
      if constexpr (DOT) { ABFT_OP(1); break; }
      return hipErrorInvalidValue;
    case 2: ABFT_OP(2); break;
    case 3: ABFT_OP(3); break;
    case 4: ABFT_OP(4); break;
    case 5: ABFT_OP(5); break;
    case 6: ABFT_OP(6); break;
    case 7: ABFT_OP(7); break;
    case 8: ABFT_OP(8); break;
    default: return hipErrorInvalidValue;
  }
#undef ABFT_OP
  return hipGetLastError();
}

template <bool DOT, bool VECC = false>
static hipError_t launch_spmm_csr_any(int mode, int k, const CsrDev &A, const double *x, double *y, EventRing ev,
                                      double *dotp, hipStream_t s) {
  if (A.nblk == 0) return hipSuccess;
  switch (mode) {
    case MODE_NONE: return launch_spmm_csr_mode<MODE_NONE, DOT, VECC>(k, A, x, y, ev, dotp, s);
    case MODE_CONSTRAINTS: return launch_spmm_csr_mode<MODE_CONSTRAINTS, DOT, VECC>(k, A, x, y, ev, dotp, s);
    case MODE_SED: return launch_spmm_csr_mode<MODE_SED, DOT, VECC>(k, A, x, y, ev, dotp, s);
    case MODE_SEC7: return launch_spmm_csr_mode<MODE_SEC7, DOT, VECC>(k, A, x, y, ev, dotp, s);
    case MODE_SEC8: return launch_spmm_csr_mode<MODE_SEC8, DOT, VECC>(k, A, x, y, ev, dotp, s);
    case MODE_SECDED: return launch_spmm_csr_mode<MODE_SECDED, DOT, VECC>(k, A, x, y, ev, dotp, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_spmm_csr(int mode, int k, const CsrDev &A, const double *x, double *y, EventRing ev,
                           hipStream_t s) {
  return launch_spmm_csr_any<false>(mode, k, A, x, y, ev, nullptr, s);
}

hipError_t launch_spmm_dot_csr(int mode, int k, const CsrDev &A, const double *x, double *y, EventRing ev,
                               double *dotp, hipStream_t s) {
  return launch_spmm_csr_any<true>(mode, k, A, x, y, ev, dotp, s);
}

hipError_t launch_spmm_dot_vecc_csr(int mode, int k, const CsrDev &A, const double *x, double *y, EventRing ev,
                                    double *dotp, hipStream_t s) {
  return launch_spmm_csr_any<true, true>(mode, k, A, x, y, ev, dotp, s);
}

// ----------------------------------------------------------------- COO SpMV --

// Load phase for COO: one 16-byte element per lane per step (1 KiB per wave
// instruction), ECC over the 4 words, gather x[row], park value*x in LDS.
// Constraints mode (reference COO/CPUContext.cpp:155-188) compares with the
// caller-order successor, reached through the two permutation arrays.
// Also parks the element's column -- masked in the ECC modes, after any repair: the
// output the reference adds the product to (COO/CPUContext.cpp:120, :224, :267, :320,
// :376) -- so that the summing phase can tell an element whose column no longer names
// the group it is stored in (see MovedList).
// Constraints mode, COO (reference COO/CPUContext.cpp:155-188): element i of the CALLER's order is checked for its
// sizes and against element i + 1 -- which the grouped storage keeps somewhere else: reading it for every element is
// one HBM-served gather per element (rounds 2-3: 3.1-3.6 x the time of `none` on scattered matrices).  Instead:
// the outcome of a pair's check can only differ from what it was at create time if one of its two elements has
// changed since, and an element that has changed no longer equals the copy of its {col,row} taken then
// (CooDev::as_created).  So the hot path compares each element with its copy, and an element that differs runs the
// reference's checks on the words as STORED NOW for both pairs it is part of: its own chain (sizes, then the pair
// with its successor), and its predecessor's pair with it -- unless the predecessor differs from its copy too and
// therefore runs that pair itself.  Every pair with a changed member is checked exactly once, on the stored words;
// a pair with none passes as it did at create time.  (An element whose checks FAIL at create time gets the
// complement of its words as the copy: it never matches and is checked on every pass.)  A fault in the copy itself
// costs a visit here and finds nothing: the verdicts only ever come from the matrix' own words.
__device__ __forceinline__ bool coo_constraints_cold(const CooDev &A, const EventRing &ev, uint32_t j) {
  const uint2 me = *reinterpret_cast<const uint2 *>(A.elems + j);
  const uint32_t col = me.x, row = me.y, oi = A.orig_index[j];
  int kind = 0;
  if (row >= A.n_in) kind = ABFT_EV_ROW_SIZE;
  else if (col >= A.n_out) kind = ABFT_EV_COL_SIZE;
  else if (oi + 1u < A.nnz) {  // (the last element has no successor: COO/CPUContext.cpp:168)
    const uint2 nx = *reinterpret_cast<const uint2 *>(A.elems + A.pos_of_orig[oi + 1u]);
    if (row > nx.y) kind = ABFT_EV_ROW_ORDER;
    else if (row == nx.y && col >= nx.x) kind = ABFT_EV_COL_ORDER;
  }
  if (kind) push_event(ev, (uint32_t)kind, event_index(A, j), 0, FMT_COO);
  if (oi >= 1u) {
    const uint32_t pj = A.pos_of_orig[oi - 1u];
    const uint2 pe = *reinterpret_cast<const uint2 *>(A.elems + pj);
    const uint2 pm = A.as_created[pj];
    if (pe.x == pm.x && pe.y == pm.y) {  // an unchanged predecessor (its sizes hold, as at create time) does not come here itself
      int pk = 0;
      if (pe.y > row) pk = ABFT_EV_ROW_ORDER;
      else if (pe.y == row && pe.x >= col) pk = ABFT_EV_COL_ORDER;
      if (pk) push_event(ev, (uint32_t)pk, event_index(A, pj), 0, FMT_COO);
    }
  }
  return kind == 0;
}

template <int EPT> struct CooTileRegs {
  u32x4 e[EPT];
  u32x2 made[EPT];  // constraints mode: the elements' {col,row} as created (coo_constraints_cold); unused otherwise
};

// the streaming loads of one COO tile [lo, hi): out-of-tile lanes re-read its first element
template <int MODE, int EPT>
__device__ __forceinline__ void coo_issue_loads(const CooDev &A, uint32_t lo, uint32_t hi, CooTileRegs<EPT> &t) {
#pragma unroll
  for (int s = 0; s < EPT; s++) {
    const uint32_t j = lo + threadIdx.x + (uint32_t)s * ABFT_BLOCK;
    t.e[s] = STREAM_LOAD(reinterpret_cast<const u32x4 *>(A.elems + (j < hi ? j : lo)));
    if (MODE == MODE_CONSTRAINTS) t.made[s] = STREAM_LOAD(reinterpret_cast<const u32x2 *>(A.as_created) + (j < hi ? j : lo));
  }
  // Keep every streaming load ahead of the first use.  Without this hipcc is free to put an element's
  // range check right behind its load -- and in `none`, where nothing else sits between them, it does:
  // load, s_waitcnt vmcnt(0), load, ... four HBM round trips per tile in a row (config 5 `none`: 227 us
  // against 194 us in `sed`).  In the ECC modes the barrier measured 3 % slower (round 1), so it is
  // per mode: ABFT_CFG_COO_SCHED_BARRIER bit m = mode m.
  if ((ABFT_CFG_COO_SCHED_BARRIER >> MODE) & 1) __builtin_amdgcn_sched_barrier(0);
}

// ECC, gathers, products and columns -> LDS for a tile whose loads were issued into `t`;
// `prefetch`: the next tile's streaming loads go out right behind this tile's gathers.
template <int MODE, int EPT>
__device__ __forceinline__ void coo_consume(const CooDev &A, const double *__restrict__ x, const EventRing &ev,
                                            uint32_t lo, uint32_t hi, const CooTileRegs<EPT> &t, double *s_prod,
                                            uint32_t *s_col, bool prefetch, uint32_t nlo, uint32_t nhi,
                                            CooTileRegs<EPT> &nxt) {
  uint32_t row[EPT];
  double val[EPT];
  bool ok[EPT];
  uint32_t changed = 0u;  // constraints mode: bit s = element s of this lane differs from its copy
  // constraints mode compares every element with its successor in the CALLER's order (reference
  // COO/CPUContext.cpp:170-186), which sits somewhere else in the grouped storage: see coo_constraints_cold.
  // Hot path: the element's {col,row} against what create_matrix stored (one coalesced 8-byte load beside the element's).
#pragma unroll
  for (int s = 0; s < EPT; s++) {
    const uint32_t j = lo + threadIdx.x + (uint32_t)s * ABFT_BLOCK;
    uint32_t w[4] = {t.e[s].x, t.e[s].y, t.e[s].z, t.e[s].w};
    bool valid = j < hi;
    if (MODE == MODE_CONSTRAINTS) {
      // (only noted here: the checks run behind the LDS writes, where nothing of the tile is live any more -- with
      // them, or a call to them, in this loop the kernel took 565 instead of 267 us on the 5-point Laplacian)
      if (valid && (w[0] != t.made[s].x || w[1] != t.made[s].y)) changed |= 1u << s;
    } else if (MODE >= MODE_SED) {
#ifdef ABFT_DBG_NOCOLD
      if (__builtin_expect(valid && ecc_suspect<FMT_COO, MODE>(w) != 0, 0)) valid = false;
      if (false) {
#else
      if (__builtin_expect(valid && ecc_suspect<FMT_COO, MODE>(w) != 0, 0)) {
#endif
        EccWords<FMT_COO> ce;
        ce.w[0] = w[0]; ce.w[1] = w[1]; ce.w[2] = w[2]; ce.w[3] = w[3]; ce.rc = 0;
        ce = ecc_cold<FMT_COO, MODE>(ce, event_index(A, j), ev);
        w[0] = ce.w[0]; w[1] = ce.w[1]; w[2] = ce.w[2]; w[3] = ce.w[3];
        if (ce.rc > 0) A.elems[j] = make_uint4(w[0], w[1], w[2], w[3]);  // COO/CPUContext.cpp:255, 310, 364
        else valid = false;
      }
    }
    row[s] = w[1];
    val[s] = as_double(w[2], w[3]);
    ok[s] = valid;
    s_col[threadIdx.x + (uint32_t)s * ABFT_BLOCK] = MODE >= MODE_SED ? (w[0] & ABFT_COLMASK) : w[0];
  }
  double xv[EPT];
#pragma unroll
  for (int s = 0; s < EPT; s++) {
    const bool in = ok[s] && row[s] < A.n_in;
#ifdef ABFT_DBG_NOGATHER  // timing-only build: wrong results
    xv[s] = (double)row[s];
#else
    xv[s] = gather_load(x + (in ? row[s] : 0u));
#endif
    xv[s] = in ? xv[s] : 0.0;
  }
  if (prefetch) coo_issue_loads<MODE, EPT>(A, nlo, nhi, nxt);
#pragma unroll
  for (int s = 0; s < EPT; s++) {
    const double p = val[s] * xv[s];
    s_prod[threadIdx.x + (uint32_t)s * ABFT_BLOCK] = ok[s] ? p : 0.0;
  }
#ifndef ABFT_DBG_NOCOLD  // (timing-only build without the checks of changed elements)
  if (MODE == MODE_CONSTRAINTS && __builtin_expect(changed != 0u, 0)) {
#pragma unroll 1
    for (uint32_t s = 0; s < (uint32_t)EPT; s++) {
      if (!((changed >> s) & 1u)) continue;
      // (an element that violates a constraint contributes nothing: the reference has stopped in front of it)
      if (!coo_constraints_cold(A, ev, lo + threadIdx.x + s * ABFT_BLOCK)) s_prod[threadIdx.x + s * ABFT_BLOCK] = 0.0;
    }
  }
#endif
}

template <int MODE, int EPT>
__device__ __forceinline__ void coo_stage(const CooDev &A, const double *__restrict__ x,
                                          const EventRing &ev, uint32_t lo, uint32_t hi,
                                          double *s_prod, uint32_t *s_col) {
  CooTileRegs<EPT> t, unused;
  coo_issue_loads<MODE, EPT>(A, lo, hi, t);
  coo_consume<MODE, EPT>(A, x, ev, lo, hi, t, s_prod, s_col, false, 0u, 0u, unused);
}

// the same for a PRODUCER wave of spmv_coo_pc_kernel: `tid` = index among the 256 producer threads, loads already in `t`.
// The cold path is kept OUT of the hot section: an element that fails its check is staged as "no product" and only
// flagged; behind the LDS writes, where nothing of the tile is live in registers any more, a wave with a flagged lane
// re-reads those elements, repairs them (ecc_cold: out of line) and overwrites their two LDS slots -- the consumers
// see the buffer only after that.  (A call inside the hot section costs the callee's registers on top of everything
// live across it: 88 VGPRs against 64 here.)
template <int MODE, int EPT>
__device__ __forceinline__ void coo_consume_pc(const CooDev &A, const double *__restrict__ x, const EventRing &ev,
                                               uint32_t lo, uint32_t hi, const CooTileRegs<EPT> &t, double *s_prod,
                                               uint32_t *s_col, uint32_t tid) {
  uint32_t row[EPT];
  double val[EPT];
  bool ok[EPT];
  uint32_t sus = 0u;  // bit s: element s failed its check
#pragma unroll
  for (int s = 0; s < EPT; s++) {
    const uint32_t j = lo + tid + (uint32_t)s * ABFT_BLOCK;
    const uint32_t w[4] = {t.e[s].x, t.e[s].y, t.e[s].z, t.e[s].w};
    bool valid = j < hi;
    if (MODE >= MODE_SED) {
      if (valid && ecc_suspect<FMT_COO, MODE>(w) != 0) {
        sus |= 1u << s;
        valid = false;
      }
    }
    row[s] = w[1];
    val[s] = as_double(w[2], w[3]);
    ok[s] = valid;
    s_col[tid + (uint32_t)s * ABFT_BLOCK] = MODE >= MODE_SED ? (w[0] & ABFT_COLMASK) : w[0];
  }
  double xv[EPT];
#pragma unroll
  for (int s = 0; s < EPT; s++) {
    const bool in = ok[s] && row[s] < A.n_in;
#ifdef ABFT_DBG_NOGATHER  // timing-only build: wrong results
    xv[s] = (double)row[s];
#else
    xv[s] = gather_load(x + (in ? row[s] : 0u));
#endif
    xv[s] = in ? xv[s] : 0.0;
  }
#pragma unroll
  for (int s = 0; s < EPT; s++) {
    const double p = val[s] * xv[s];
    s_prod[tid + (uint32_t)s * ABFT_BLOCK] = ok[s] ? p : 0.0;
  }
  if (MODE >= MODE_SED && __builtin_expect(__builtin_amdgcn_ballot_w64(sus != 0u) != 0ull, 0)) {
    for (int s = 0; s < EPT; s++) {  // (not unrolled: one call site)
      if (!((sus >> s) & 1u)) continue;
      const uint32_t j = lo + tid + (uint32_t)s * ABFT_BLOCK;
      const uint4 el = A.elems[j];
      EccWords<FMT_COO> ce;
      ce.w[0] = el.x; ce.w[1] = el.y; ce.w[2] = el.z; ce.w[3] = el.w; ce.rc = 0;
      ce = ecc_cold<FMT_COO, MODE>(ce, event_index(A, j), ev);
      double p = 0.0;
      if (ce.rc > 0) {
        A.elems[j] = make_uint4(ce.w[0], ce.w[1], ce.w[2], ce.w[3]);  // COO/CPUContext.cpp:255, 310, 364
        const bool in = ce.w[1] < A.n_in;
        const double xr = gather_load(x + (in ? ce.w[1] : 0u));
        p = as_double(ce.w[2], ce.w[3]) * (in ? xr : 0.0);
      }
      s_col[tid + (uint32_t)s * ABFT_BLOCK] = ce.w[0] & ABFT_COLMASK;
      s_prod[tid + (uint32_t)s * ABFT_BLOCK] = p;
    }
  }
}

// Cold: the product staged at LDS slot k (stored position j) belongs to output `col`,
// not to the group it is stored in.  Queue it for coo_fixup_kernel; a column outside
// the result vector is dropped (the reference writes out of bounds there: undefined).
// (everything by value, in registers: a reference to the kernel's CooDev would put the
// whole argument struct into scratch memory and the hot path would read it from there)
__device__ __noinline__ void coo_push_moved_cold(MovedEntry *buf, uint32_t *count, uint32_t cap,
                                                 const uint32_t *orig_index, abft_event *evbuf, uint32_t *evcount,
                                                 uint32_t evcap, uint32_t j, uint32_t col, double prod) {
  const uint32_t slot = atomicAdd(count, 1u);
  if (slot < cap) {
    MovedEntry m;
    m.orig = orig_index[j]; m.col = col; m.prod = prod;
    buf[slot] = m;
  } else if (slot == cap) {
    EventRing ev;
    ev.buf = evbuf; ev.count = evcount; ev.cap = evcap;
    push_event(ev, ABFT_EV_MOVED_OVERFLOW, cap, 0, FMT_COO);
  }
}
__device__ __forceinline__ void coo_push_moved(const CooDev &A, const EventRing &ev, uint32_t j, uint32_t col,
                                               double prod) {
  if (col < A.n_out)
    coo_push_moved_cold(A.moved.buf, A.moved.count, A.moved.cap, A.orig_index, ev.buf, ev.count, ev.cap, j, col, prod);
}

// Continue the ordered sum of output `out` over LDS slots [a, b) from `acc`: four reads
// in flight, adds in slot order.  A slot whose staged column is not `out` is left out of
// the sum (no "+ 0.0") and queued for the fix-up; `j0` = stored position of slot 0.
template <bool SHORT = false>
__device__ __forceinline__ void lds_ordered_add(const CooDev &A, const EventRing &ev, const double *s_prod,
                                                const uint32_t *s_col, uint32_t a, uint32_t b, uint32_t out,
                                                uint32_t j0, double &acc) {
  if (SHORT) {  // the panel kernel's ranges (an output's elements inside one panel and tile) are short: two-wide
    for (uint32_t k = a; k < b; k += 2u) {
      const uint32_t last = b - 1u, k1 = min(k + 1u, last);
      const double a0 = s_prod[k], a1 = s_prod[k1];
      const uint32_t c0 = s_col[k], c1 = s_col[k1];
      if (c0 == out) acc += a0;
      if (k + 1u < b && c1 == out) acc += a1;
      if (__builtin_expect(((c0 ^ out) | (c1 ^ out)) != 0u, 0)) {
        if (c0 != out) coo_push_moved(A, ev, j0 + k, c0, a0);
        if (k + 1u < b && c1 != out) coo_push_moved(A, ev, j0 + k + 1u, c1, a1);
      }
    }
    return;
  }
  for (uint32_t k = a; k < b; k += 4u) {
    const uint32_t last = b - 1u;
    const uint32_t k1 = min(k + 1u, last), k2 = min(k + 2u, last), k3 = min(k + 3u, last);
    const double a0 = s_prod[k], a1 = s_prod[k1], a2 = s_prod[k2], a3 = s_prod[k3];
    const uint32_t c0 = s_col[k], c1 = s_col[k1], c2 = s_col[k2], c3 = s_col[k3];
    if (c0 == out) acc += a0;
    if (k + 1u < b && c1 == out) acc += a1;
    if (k + 2u < b && c2 == out) acc += a2;
    if (k + 3u < b && c3 == out) acc += a3;
    if (__builtin_expect(((c0 ^ out) | (c1 ^ out) | (c2 ^ out) | (c3 ^ out)) != 0u, 0)) {
      if (c0 != out) coo_push_moved(A, ev, j0 + k, c0, a0);
      if (k + 1u < b && c1 != out) coo_push_moved(A, ev, j0 + k + 1u, c1, a1);
      if (k + 2u < b && c2 != out) coo_push_moved(A, ev, j0 + k + 2u, c2, a2);
      if (k + 3u < b && c3 != out) coo_push_moved(A, ev, j0 + k + 3u, c3, a3);
    }
  }
}

// The consumer waves' form (spmv_coo_pc_kernel), two-wide: a stranger is noted in a small per-wave LDS list
// {stored position, column, product} instead of being queued from here -- the out-of-line queueing call would cost
// the hot loop its callee's registers (98 VGPRs against 62) -- and the wave queues its list once its group is done.
struct MovedNote { uint32_t j, col; double prod; };
constexpr uint32_t PC_NOTES = 32;  // per consumer wave and group; more than that in one group: ABFT_EV_MOVED_OVERFLOW
__device__ __forceinline__ void lds_ordered_add_pc(const double *s_prod, const uint32_t *s_col, uint32_t a, uint32_t b,
                                                   uint32_t out, uint32_t j0, double &acc, uint32_t *s_ncount,
                                                   MovedNote *s_notes) {
  for (uint32_t k = a; k < b; k += 2u) {
    const uint32_t last = b - 1u, k1 = min(k + 1u, last);
    const double a0 = s_prod[k], a1 = s_prod[k1];
    const uint32_t c0 = s_col[k], c1 = s_col[k1];
    if (c0 == out) acc += a0;
    if (k + 1u < b && c1 == out) acc += a1;
    if (__builtin_expect(((c0 ^ out) | (c1 ^ out)) != 0u, 0)) {
      if (c0 != out) {
        const uint32_t n = atomicAdd(s_ncount, 1u);
        if (n < PC_NOTES) { s_notes[n].j = j0 + k; s_notes[n].col = c0; s_notes[n].prod = a0; }
      }
      if (k + 1u < b && c1 != out) {
        const uint32_t n = atomicAdd(s_ncount, 1u);
        if (n < PC_NOTES) { s_notes[n].j = j0 + k + 1u; s_notes[n].col = c1; s_notes[n].prod = a1; }
      }
    }
  }
}

// COO SpMV, all modes: result[col] += value * vec[row] (reference
// COO/CPUContext.cpp:104-121).  Elements are stored grouped by col in caller
// order, so an output's contributions are added in exactly the order the
// reference's serial loop adds them; the workgroup/tile structure is the CSR
// one with (group, grp_ptr) in place of (row, rowptr).
template <int MODE, int EPT, bool FUSE>
__global__ __launch_bounds__(ABFT_BLOCK) void spmv_coo_kernel(CooDev A, const double *__restrict__ x,
                                                              double *__restrict__ y, EventRing ev,
                                                              FuseOut fuse) {
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  __shared__ __attribute__((aligned(16))) double s_prod[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[TILE];
  const uint32_t t = xcd_tile(blockIdx.x, A.nblk);
  const uint4 desc = A.blk[t];
  const uint32_t g0 = desc.x, g1 = desc.y, e0 = desc.z, e1 = desc.w;
  double dsum = 0.0;

  if (e1 - e0 <= TILE) {
    const uint32_t g = g0 + threadIdx.x;
    uint32_t gs = 0, ge = 0;
    double xg = 0.0;
    if (g < g1) {
      gs = A.grp_ptr[g]; ge = A.grp_ptr[g + 1];  // (the uniform-block shortcut of the CSR kernel measured 4 % slower here)
      if (FUSE) xg = x[fuse.x_off + g];
    }
    coo_stage<MODE, EPT>(A, x, ev, e0, e1, s_prod, s_col);
    __syncthreads();
    for (uint32_t grp = g; grp < g1; grp += ABFT_BLOCK) {
      if (grp != g) {
        gs = A.grp_ptr[grp]; ge = A.grp_ptr[grp + 1];
        if (FUSE) xg = x[fuse.x_off + grp];
      }
      // reference zero-fills result first (COO/CPUContext.cpp:108-109)
      double acc = 0.0;
      lds_ordered_add(A, ev, s_prod, s_col, gs - e0, ge - e0, grp, e0, acc);
      y[grp] = acc;
      if (FUSE) dsum += xg * acc;
    }
  } else {
    for (uint32_t grp = g0; grp < g1; grp++) {  // a group longer than a tile
      const uint32_t gs = A.grp_ptr[grp], ge = A.grp_ptr[grp + 1];
      double acc = 0.0;
      for (uint32_t lo = gs; lo < ge;) {
        const uint32_t hi = min(ge, lo + TILE);
        __syncthreads();
        coo_stage<MODE, EPT>(A, x, ev, lo, hi, s_prod, s_col);
        __syncthreads();
        if (threadIdx.x == 0) lds_ordered_add(A, ev, s_prod, s_col, 0u, hi - lo, grp, lo, acc);
        lo = hi;
      }
      if (threadIdx.x == 0) {
        y[grp] = acc;
        if (FUSE) dsum += x[fuse.x_off + grp] * acc;
      }
    }
  }
  if (FUSE) fused_dot_finish(dsum, fuse, blockIdx.x);
}

// ---- pacing helpers (used by the COO panel kernel and the sweep / slice kernels) ----
// pace buffer: per XCD a board of PACE_SLOTS progress words (steps completed by the workgroup
// that owns that slot; ~0u = nobody there, which is also how every workgroup leaves its slot)
constexpr uint32_t PACE_SLOTS = 256;

// which of the 8 XCDs (each with its own L2) this wave runs on
__device__ __forceinline__ uint32_t xcc_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 7u;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true);
}

// inclusive prefix sum over the 64 lanes, entirely in the VALU (same steps as wave_sum:
// Hillis-Steele inside each 16-lane row, then the row totals carried across)
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v) {
  v += dpp_u32<0x111, 0xf>(v);
  v += dpp_u32<0x112, 0xf>(v);
  v += dpp_u32<0x114, 0xf>(v);
  v += dpp_u32<0x118, 0xf>(v);
  v += dpp_u32<0x142, 0xa>(v);
  v += dpp_u32<0x143, 0xc>(v);
  return v;
}

// Pacing (speed only, never correctness).  What keeps the workgroups of an XCD inside one
// window of the gathered vector -- so that the XCD's L2 serves the gathers -- is a progress
// board per XCD: every workgroup publishes the number of panel steps it has completed with a
// plain store (write-through to the XCD's L2) and reads the whole board of ITS XCD with one
// wave-wide L1-bypassing load (256 words = 4 per lane), served by that same L2; the minimum
// says how far the slowest workgroup of the XCD is.  Nothing crosses the fabric per step
// (agent-scope atomics did: ~5 us each under load, measured, more than the misses cost),
// no data is handed over (no fences), and every wait is bounded.
struct BoardView { uint64_t a, b; };  // this lane's four progress words

__device__ __forceinline__ BoardView board_load(const uint32_t *board, uint32_t lane) {
  const uint64_t *p = reinterpret_cast<const uint64_t *>(board) + 2u * lane;
  BoardView v;
  v.a = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v.b = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_min_step(uint32_t v) {  // lanes without a source keep their own value
  return min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false));
}

// minimum over the board (wave-uniform result)
__device__ __forceinline__ uint32_t board_min(const BoardView &v) {
  uint32_t m = min(min((uint32_t)v.a, (uint32_t)(v.a >> 32)), min((uint32_t)v.b, (uint32_t)(v.b >> 32)));
  m = dpp_min_step<0x111>(m);  // row_shr 1, 2, 4, 8: lane 15 of each 16-lane row holds the row's minimum
  m = dpp_min_step<0x112>(m);
  m = dpp_min_step<0x114>(m);
  m = dpp_min_step<0x118>(m);
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)m, 15), r1 = (uint32_t)__builtin_amdgcn_readlane((int)m, 31),
                 r2 = (uint32_t)__builtin_amdgcn_readlane((int)m, 47), r3 = (uint32_t)__builtin_amdgcn_readlane((int)m, 63);
  return min(min(r0, r1), min(r2, r3));
}


#ifdef ABFT_DBG_STAMPS  // timing build: where a workgroup's time goes (wave 0's clock), summed into the layout's debug words (sweep: L.debug[4..9], COO panels: P.debug[0..7])
#define STAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory")
#define STAMP_ADD(slot, a, b) dbg_t[slot] += (b) - (a)
#else
#define STAMP(var)
#define STAMP_ADD(slot, a, b)
#endif

// Panel-layout COO SpMV: the CSR panel kernel with (output group, row panel)
// segments of 16-byte elements; outputs are the reference's result[col], the
// gather index is the element's row (COO/CPUContext.cpp:111-120).
template <int MODE, int EPT, bool FUSE>
__global__ __launch_bounds__(ABFT_BLOCK) void spmv_coo_panels_kernel(CooDev A, CsrPanels P,
                                                                     const double *__restrict__ x,
                                                                     double *__restrict__ y, EventRing ev,
                                                                     FuseOut fuse, uint32_t c0, uint32_t c1) {
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  constexpr int RPT = ABFT_PANEL_ROWS_PER_THREAD;
  __shared__ __attribute__((aligned(16))) double s_prod[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[TILE];
  double dsum = 0.0;
  // Pacing, as in the sweep kernel (speed only, every wait bounded): with all panels in one launch what keeps the
  // workgroups of an XCD inside one window of x is a progress board per XCD -- a workgroup starts panel step s
  // only when the slowest of its XCD has completed step s - lag.
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nsteps = c1 - c0;
  const bool pace = P.pace != nullptr && P.lag != 0u;
  uint32_t *board = nullptr;
  uint32_t my_slot = 0xffffffffu;
  if (pace) {
    board = P.pace + xcc_id() * PACE_SLOTS;
    if (wave == 0u) {
      my_slot = blockIdx.x >> 3;  // workgroups are dealt to the XCDs round-robin: distinct slots on a board
      if (lane == 0u && my_slot < PACE_SLOTS) board[my_slot] = 0u;
    }
  }
  BoardView seen{~0ull, ~0ull};
  bool have_seen = false, gave_up = false;
  uint32_t round = 0;
#ifdef ABFT_DBG_STAMPS
  // [0] segment tables (seg_base, 16-bit offsets)  [1] barrier in front of a tile  [2] staging (loads, ECC, gathers,
  // LDS writes)  [3] barrier behind it  [4] ordered adds  [5] y prologue  [6] y epilogue + fused product  [7] total
  unsigned long long dbg_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  STAMP(t_begin);
#endif
  for (uint32_t g = blockIdx.x; g < P.ngroups; g += gridDim.x, round++) {
    const uint32_t out0 = g * ABFT_PANEL_ROWS;
    double acc[RPT];
    STAMP(t_p0);
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t o = out0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x;
      acc[j] = (c0 > 0 && o < A.n_out) ? y[o] : 0.0;
    }
#ifdef ABFT_DBG_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    STAMP(t_p1);
    STAMP_ADD(5, t_p0, t_p1);
    for (uint32_t c = c0; c < c1; c++) {
      STAMP(t_s0);
      const uint32_t seg = g * P.npanels + c;
      const uint32_t e0 = P.seg_base[seg], e1 = P.seg_base[seg + 1];
      const uint32_t step = round * nsteps + (c - c0);
      if (e0 == e1) {  // uniform
        if (pace && threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = step + 1u;
        continue;
      }
      if (pace && wave == 0u) {
        if (step >= P.lag && !gave_up) {
          const uint32_t need = step + 1u - P.lag;
          uint32_t m = have_seen ? board_min(seen) : 0u;
          if (m < need) {
            int it = 0;
            for (; it < 1024 && m < need; it++) {
              __builtin_amdgcn_s_sleep(4);
              m = board_min(board_load(board, lane));
            }
            if (it == 1024) gave_up = true;  // ~1 ms and still short: stop pacing rather than stall again
          }
        }
        seen = board_load(board, lane);  // for the next step: its latency runs beside this step's work
        have_seen = true;
      }
      const uint16_t *ptr = P.seg_ptr + (size_t)seg * (ABFT_PANEL_ROWS + 1);
      uint32_t gs[RPT], ge[RPT];
#pragma unroll
      for (int j = 0; j < RPT; j++) {
        const uint32_t r = (uint32_t)j * ABFT_BLOCK + threadIdx.x;
        gs[j] = e0 + ptr[r];
        ge[j] = e0 + ptr[r + 1];
      }
      // x prefetch: every gather of a tile waits for the slowest of its 1024, and 4-7 % of them miss the XCD's L2
      // (each line of x must come into each L2 once per SpMV: 1.05 M of config 5's 26 M gathers, plus re-fetches) --
      // so EVERY tile pays a miss's latency.  Entering panel c the workgroups of an XCD (slot = blockIdx / 8, dealt
      // round-robin) share out the lines of panel c + AHEAD and touch one word of each: one extra load per thread, in
      // flight beside the first tile's own loads, its value unused.
      double xpf_v = 0.0;
      bool xpf_on = false;
      if (P.xpf) {
        const uint32_t cn = c + (uint32_t)ABFT_CFG_COO_PANEL_XPF_AHEAD;
        if (cn < P.npanels) {
          const uint32_t lines = (P.width + 15u) / 16u, nwg = (gridDim.x + 7u) / 8u;
          const uint32_t per = (lines + nwg - 1u) / nwg;
          const uint32_t line = (blockIdx.x >> 3) * per + threadIdx.x;
          const uint64_t row = (uint64_t)cn * P.width + (uint64_t)line * 16u;
          xpf_on = threadIdx.x < per && line < lines && row < A.n_in;
          if (xpf_on) xpf_v = gather_load(x + row);
        }
      }
#ifdef ABFT_DBG_STAMPS
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
      STAMP(t_s1);
      STAMP_ADD(0, t_s0, t_s1);
#if ABFT_CFG_COO_PANEL_PREFETCH
      // software pipeline inside a segment: tile k + 1's streaming loads go out right behind tile k's gathers and
      // are in flight during its barrier and ordered adds (16 more registers per thread)
      CooTileRegs<EPT> cur, nxt;
      coo_issue_loads<MODE, EPT>(A, e0, min(e1, e0 + TILE), cur);
#endif
      for (uint32_t lo = e0; lo < e1;) {
        const uint32_t hi = min(e1, lo + TILE);
        STAMP(t_a);
        __syncthreads();
        STAMP(t_b);
#if ABFT_CFG_COO_PANEL_PREFETCH
        coo_consume<MODE, EPT>(A, x, ev, lo, hi, cur, s_prod, s_col, hi < e1, hi, min(e1, hi + TILE), nxt);
        cur = nxt;
#else
        coo_stage<MODE, EPT>(A, x, ev, lo, hi, s_prod, s_col);
#endif
        STAMP(t_c);
        __syncthreads();
        STAMP(t_d);
#ifdef ABFT_DBG_NOADDS  // timing-only build (wrong results): one LDS read per thread instead of the ordered adds
        acc[0] += s_prod[threadIdx.x];
#else
#pragma unroll
        for (int j = 0; j < RPT; j++) {
          const uint32_t a0 = max(gs[j], lo), a1 = min(ge[j], hi);
          if (a0 < a1) {
            double t = acc[j];
            lds_ordered_add<ABFT_CFG_COO_PANEL_SHORT_SUMS>(A, ev, s_prod, s_col, a0 - lo, a1 - lo,
                                                           out0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x, lo, t);
            acc[j] = t;
          }
        }
#endif
        STAMP(t_e);
        STAMP_ADD(1, t_a, t_b);
        STAMP_ADD(2, t_b, t_c);
        STAMP_ADD(3, t_c, t_d);
        STAMP_ADD(4, t_d, t_e);
        lo = hi;
      }
      if (xpf_on) asm volatile("" ::"v"(xpf_v));  // (keeps the prefetch load; long since returned)
      if (pace && threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = step + 1u;  // plain store: into this XCD's L2
    }
    STAMP(t_q0);
    // (the fused product's operands first, all in flight together: read inside the loop below hipcc waits for each
    // before it issues the next -- RPT trips to memory in a row at the end of every workgroup)
    double xo[FUSE ? RPT : 1];
    if (FUSE) {
#pragma unroll
      for (int j = 0; j < RPT; j++) xo[j] = x[fuse.x_off + min(out0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x, A.n_out - 1u)];
    }
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t o = out0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x;
      if (o < A.n_out) {
        y[o] = acc[j];
        if (FUSE) dsum += xo[j] * acc[j];
      }
    }
    STAMP(t_q1);
    STAMP_ADD(6, t_q0, t_q1);
  }
  if (FUSE) fused_dot_finish(dsum, fuse, blockIdx.x);
  // done: never holds anyone back, and the board is clean for the next launch
  if (pace && threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = 0xffffffffu;
#ifdef ABFT_DBG_STAMPS
  if (threadIdx.x == 0 && P.debug) {
    STAMP(t_end);
    dbg_t[7] = t_end - t_begin;
    for (int k = 0; k < 8; k++) atomicAdd(P.debug + (c0 > 0 ? 8 : 0) + k, dbg_t[k]);
  }
#endif
}

// ---- the COO panel kernel with its cold paths out of the hot loop (round 4) ----
// spmv_coo_panels_kernel needs 86-89 VGPRs, of which ~30 are the price of two out-of-line calls inside its hot
// sections (the ECC repair in the staging phase, the queueing of a stranger in the summing phase: a call costs its
// callee's registers on top of everything live across it).  Here both are deferred -- a failed check is staged as "no
// product" and repaired behind the LDS writes (coo_consume_pc), a stranger is noted in a per-wave LDS list and queued
// when the group is done (lds_ordered_add_pc) -- so that the kernel fits the register budget of 8 workgroups per CU
// (with 4 outputs per thread: -DABFT_CFG_PANEL_RPT=4), i.e. twice the waves to keep gathers in flight.  Same lanes,
// same order of additions, same bits.
template <int MODE, int EPT, bool FUSE>
__global__ __launch_bounds__(ABFT_BLOCK, ABFT_CFG_COO_LEAN_WAVES) void spmv_coo_lean_kernel(CooDev A, CsrPanels P,
                                                                     const double *__restrict__ x,
                                                                     double *__restrict__ y, EventRing ev,
                                                                     FuseOut fuse, uint32_t c0, uint32_t c1) {
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  constexpr int RPT = ABFT_PANEL_ROWS_PER_THREAD;
  __shared__ __attribute__((aligned(16))) double s_prod[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[TILE];
  __shared__ MovedNote s_notes[4][PC_NOTES];
  __shared__ uint32_t s_ncount[4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < 4u) s_ncount[threadIdx.x] = 0u;
  const uint32_t nsteps = c1 - c0;
  const bool pace = P.pace != nullptr && P.lag != 0u;
  uint32_t *board = nullptr;
  uint32_t my_slot = 0xffffffffu;
  if (pace) {
    board = P.pace + xcc_id() * PACE_SLOTS;
    if (wave == 0u) {
      my_slot = blockIdx.x >> 3;
      if (lane == 0u && my_slot < PACE_SLOTS) board[my_slot] = 0u;
    }
  }
  BoardView seen{~0ull, ~0ull};
  bool have_seen = false, gave_up = false;
  uint32_t round = 0;
  double dsum = 0.0;
  for (uint32_t g = blockIdx.x; g < P.ngroups; g += gridDim.x, round++) {
    const uint32_t out0 = g * ABFT_PANEL_ROWS;
    double acc[RPT];
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t o = out0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x;
      acc[j] = (c0 > 0 && o < A.n_out) ? y[o] : 0.0;
    }
    for (uint32_t c = c0; c < c1; c++) {
      const uint32_t seg = g * P.npanels + c;
      const uint32_t e0 = P.seg_base[seg], e1 = P.seg_base[seg + 1];
      const uint32_t step = round * nsteps + (c - c0);
      if (e0 != e1) {  // uniform
        if (pace && wave == 0u) {
          if (step >= P.lag && !gave_up) {
            const uint32_t need = step + 1u - P.lag;
            uint32_t m = have_seen ? board_min(seen) : 0u;
            if (m < need) {
              int it = 0;
              for (; it < 1024 && m < need; it++) {
                __builtin_amdgcn_s_sleep(4);
                m = board_min(board_load(board, lane));
              }
              if (it == 1024) gave_up = true;
            }
          }
          seen = board_load(board, lane);
          have_seen = true;
        }
        const uint16_t *ptr = P.seg_ptr + (size_t)seg * (ABFT_PANEL_ROWS + 1);
        uint32_t gse[RPT];  // an output's range inside the segment: both ends relative to e0, 16 bits each
#pragma unroll
        for (int j = 0; j < RPT; j++) {
          const uint32_t r = (uint32_t)j * ABFT_BLOCK + threadIdx.x;
          gse[j] = (uint32_t)ptr[r] | ((uint32_t)ptr[r + 1] << 16);
        }
        for (uint32_t lo = e0; lo < e1;) {
          const uint32_t hi = min(e1, lo + TILE);
          CooTileRegs<EPT> t;
#pragma unroll
          for (int k = 0; k < EPT; k++) {
            const uint32_t j = lo + threadIdx.x + (uint32_t)k * ABFT_BLOCK;
            t.e[k] = STREAM_LOAD(reinterpret_cast<const u32x4 *>(A.elems + (j < hi ? j : lo)));
          }
          __syncthreads();  // (the previous tile's sums have left the buffer)
          coo_consume_pc<MODE, EPT>(A, x, ev, lo, hi, t, s_prod, s_col, threadIdx.x);
          __syncthreads();
#pragma unroll
          for (int j = 0; j < RPT; j++) {
            const uint32_t a0 = max(e0 + (gse[j] & 0xffffu), lo), a1 = min(e0 + (gse[j] >> 16), hi);
            if (a0 < a1) {
              double tt = acc[j];
              lds_ordered_add_pc(s_prod, s_col, a0 - lo, a1 - lo, out0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x, lo, tt,
                                 &s_ncount[wave], s_notes[wave]);
              acc[j] = tt;
            }
          }
          lo = hi;
        }
      }
      if (pace && threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = step + 1u;
    }
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t o = out0 + (uint32_t)j * ABFT_BLOCK + threadIdx.x;
      if (o < A.n_out) {
        y[o] = acc[j];
        if (FUSE) dsum += x[fuse.x_off + o] * acc[j];
      }
    }
    // cold: this wave's noted strangers go to the fix-up's queue
    const uint32_t notes = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_ncount[wave]);
    if (__builtin_expect(notes != 0u, 0)) {
      for (uint32_t k = lane; k < min(notes, PC_NOTES); k += 64u)
        coo_push_moved(A, ev, s_notes[wave][k].j, s_notes[wave][k].col, s_notes[wave][k].prod);
      if (notes > PC_NOTES && lane == 0u) push_event(ev, ABFT_EV_MOVED_OVERFLOW, PC_NOTES, 0, FMT_COO);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0u) s_ncount[wave] = 0u;
    }
  }
  if (FUSE) fused_dot_finish(dsum, fuse, blockIdx.x);
  if (pace && threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = 0xffffffffu;
}

template <int MODE> static int coo_lean_occupancy() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spmv_coo_lean_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, true>, ABFT_BLOCK, 0) !=
          hipSuccess || n < 1)
    n = 1;
  return n > 8 ? 8 : n;
}
int spmv_coo_lean_blocks_per_cu(int mode) {
  switch (mode) {
    case MODE_NONE: return coo_lean_occupancy<MODE_NONE>();
    case MODE_SED: return coo_lean_occupancy<MODE_SED>();
    case MODE_SEC7: return coo_lean_occupancy<MODE_SEC7>();
    case MODE_SEC8: return coo_lean_occupancy<MODE_SEC8>();
    default: return coo_lean_occupancy<MODE_SECDED>();
  }
}

template <int MODE>
static hipError_t launch_coo_lean_mode(const CooDev &A, const CsrPanels &P, const double *x, double *y, EventRing ev,
                                       const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s) {
  if (fuse)
    hipLaunchKernelGGL((spmv_coo_lean_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, true>), dim3(grid), dim3(ABFT_BLOCK), 0, s, A, P, x, y,
                       ev, *fuse, c0, c1);
  else
    hipLaunchKernelGGL((spmv_coo_lean_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, false>), dim3(grid), dim3(ABFT_BLOCK), 0, s, A, P, x, y,
                       ev, FuseOut{}, c0, c1);
  return hipGetLastError();
}

hipError_t launch_spmv_coo_lean(int mode, const CooDev &A, const CsrPanels &P, const double *x, double *y, EventRing ev,
                                const FuseOut *fuse, uint32_t grid, uint32_t chunk, hipStream_t s) {
  if (P.ngroups == 0) return hipSuccess;
  if (chunk == 0 || chunk > P.npanels) chunk = P.npanels;
  for (uint32_t c0 = 0; c0 < P.npanels; c0 += chunk) {
    const uint32_t c1 = c0 + chunk < P.npanels ? c0 + chunk : P.npanels;
    const FuseOut *f = c1 == P.npanels ? fuse : nullptr;
    hipError_t e;
    switch (mode) {
      case MODE_NONE: e = launch_coo_lean_mode<MODE_NONE>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SED: e = launch_coo_lean_mode<MODE_SED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC7: e = launch_coo_lean_mode<MODE_SEC7>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC8: e = launch_coo_lean_mode<MODE_SEC8>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SECDED: e = launch_coo_lean_mode<MODE_SECDED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// wait until each of the four per-wave counts (LDS) has reached `want`
__device__ __forceinline__ void pc_wait_all(const uint32_t *counts, uint32_t want) {
  for (;;) {
    const uint32_t a = __hip_atomic_load(counts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint32_t b = __hip_atomic_load(counts + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint32_t c = __hip_atomic_load(counts + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint32_t d = __hip_atomic_load(counts + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (min(min(a, b), min(c, d)) >= want) return;
    __builtin_amdgcn_s_sleep(1);
  }
}

// ---- the COO panel kernel with the two halves of a tile's work on different waves (round 4) ----
// Timing builds of spmv_coo_panels_kernel on configs[4] (sec7; gpurun_out/r4/c5_ab2.txt): streaming the elements alone
// (no gathers, no sums) 84 us; with the ordered sums 146; with the gathers and no sums 186; everything 202 -- the
// phases of a tile (stream, check, gather | barrier | sum | barrier) run one after the other inside a workgroup and
// the 4 workgroups of a CU do not fill each other's gaps: the CU's gather path (~3 clocks per gathered lane) is
// busy ~3/4 of the time.  Here a workgroup is 8 waves: waves 4-7 PRODUCE (stream a tile, check it, gather, write
// products and columns into one of NB LDS buffers) and never sum, waves 0-3 CONSUME (the ordered sums of their 8
// outputs per lane, exactly as before: same lanes, same order, same bits) and never touch global memory inside a
// tile.  No workgroup barrier in the loop: two LDS counters (tiles filled x4, tiles summed x4) pace the two sides,
// so the producers of a CU keep gathers in flight while its consumers sum.  Registers: the roles' needs do not
// add up (tile registers on one side, sums and ranges on the other), 8 waves per SIMD.
template <int MODE, int EPT, bool FUSE>
__global__ __launch_bounds__(512, 8) void spmv_coo_pc_kernel(CooDev A, CsrPanels P, const double *__restrict__ x,
                                                             double *__restrict__ y, EventRing ev, FuseOut fuse,
                                                             uint32_t c0, uint32_t c1) {
  constexpr uint32_t TILE = ABFT_BLOCK * EPT;
  constexpr int RPT = ABFT_PANEL_ROWS_PER_THREAD;
  constexpr uint32_t NB = 2;  // LDS buffers
  __shared__ __attribute__((aligned(16))) double s_prod[NB][TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_col[NB][TILE];
  // tiles filled by each producer wave / summed by each consumer wave (a wave may be a tile ahead of its peers: one
  // shared count would let three fast waves stand in for a slow one)
  __shared__ __attribute__((aligned(16))) uint32_t s_full[4], s_done[4];
  __shared__ double s_w[8];
  __shared__ MovedNote s_notes[4][PC_NOTES];  // per consumer wave: products whose column names another output (cold)
  __shared__ uint32_t s_ncount[4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool producer = wave >= 4u;
  const uint32_t tid = threadIdx.x & 255u;  // index inside the role
  if (threadIdx.x < 4u) { s_full[threadIdx.x] = 0u; s_done[threadIdx.x] = 0u; s_ncount[threadIdx.x] = 0u; }
  __syncthreads();
  const uint32_t nsteps = c1 - c0;
  const bool pace = P.pace != nullptr && P.lag != 0u;
  uint32_t *board = nullptr;
  uint32_t my_slot = 0xffffffffu;
  if (pace) {
    board = P.pace + xcc_id() * PACE_SLOTS;
    if (wave == 4u) {
      my_slot = blockIdx.x >> 3;
      if (lane == 0u && my_slot < PACE_SLOTS) board[my_slot] = 0u;
    }
  }
  BoardView seen{~0ull, ~0ull};
  bool have_seen = false, gave_up = false;
  uint32_t tile_no = 0;  // tiles of this workgroup so far (both roles count alike)
  uint32_t round = 0;
  double dsum = 0.0;
  for (uint32_t g = blockIdx.x; g < P.ngroups; g += gridDim.x, round++) {
    const uint32_t out0 = g * ABFT_PANEL_ROWS;
    if (producer) {
      for (uint32_t c = c0; c < c1; c++) {
        const uint32_t seg = g * P.npanels + c;
        const uint32_t e0 = P.seg_base[seg], e1 = P.seg_base[seg + 1];
        const uint32_t step = round * nsteps + (c - c0);
        if (e0 != e1) {  // uniform
          if (pace && wave == 4u) {
            if (step >= P.lag && !gave_up) {
              const uint32_t need = step + 1u - P.lag;
              uint32_t m = have_seen ? board_min(seen) : 0u;
              if (m < need) {
                int it = 0;
                for (; it < 1024 && m < need; it++) {
                  __builtin_amdgcn_s_sleep(4);
                  m = board_min(board_load(board, lane));
                }
                if (it == 1024) gave_up = true;
              }
            }
            seen = board_load(board, lane);
            have_seen = true;
          }
          for (uint32_t lo = e0; lo < e1; tile_no++) {
            const uint32_t hi = min(e1, lo + TILE);
            const uint32_t b = tile_no % NB;
            CooTileRegs<EPT> t;
            // the streaming loads do not need the buffer: issue them, THEN wait for the consumers to have left it
#pragma unroll
            for (int k = 0; k < EPT; k++) {
              const uint32_t j = lo + tid + (uint32_t)k * ABFT_BLOCK;
              t.e[k] = STREAM_LOAD(reinterpret_cast<const u32x4 *>(A.elems + (j < hi ? j : lo)));
            }
            if (tile_no >= NB) pc_wait_all(s_done, tile_no - NB + 1u);  // every consumer wave has summed tile tile_no - NB
            coo_consume_pc<MODE, EPT>(A, x, ev, lo, hi, t, s_prod[b], s_col[b], tid);
            // this wave's LDS writes have landed: count it in
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0u) __hip_atomic_store(&s_full[wave - 4u], tile_no + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            lo = hi;
          }
        }
        if (pace && wave == 4u && lane == 0u && my_slot < PACE_SLOTS) board[my_slot] = step + 1u;
      }
    } else {
      double acc[RPT];
#pragma unroll
      for (int j = 0; j < RPT; j++) {
        const uint32_t o = out0 + (uint32_t)j * ABFT_BLOCK + tid;
        acc[j] = (c0 > 0 && o < A.n_out) ? y[o] : 0.0;
      }
      for (uint32_t c = c0; c < c1; c++) {
        const uint32_t seg = g * P.npanels + c;
        const uint32_t e0 = P.seg_base[seg], e1 = P.seg_base[seg + 1];
        if (e0 == e1) continue;  // uniform
        const uint16_t *ptr = P.seg_ptr + (size_t)seg * (ABFT_PANEL_ROWS + 1);
        uint32_t gse[RPT];  // an output's range inside the segment, both ends relative to e0 in 16 bits each (a segment holds < 65536 elements)
#pragma unroll
        for (int j = 0; j < RPT; j++) {
          const uint32_t r = (uint32_t)j * ABFT_BLOCK + tid;
          gse[j] = (uint32_t)ptr[r] | ((uint32_t)ptr[r + 1] << 16);
        }
        for (uint32_t lo = e0; lo < e1; tile_no++) {
          const uint32_t hi = min(e1, lo + TILE);
          const uint32_t b = tile_no % NB;
          pc_wait_all(s_full, tile_no + 1u);  // every producer wave has filled tile tile_no
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
          for (int j = 0; j < RPT; j++) {
            const uint32_t a0 = max(e0 + (gse[j] & 0xffffu), lo), a1 = min(e0 + (gse[j] >> 16), hi);
            if (a0 < a1) {
              double tt = acc[j];
              lds_ordered_add_pc(s_prod[b], s_col[b], a0 - lo, a1 - lo, out0 + (uint32_t)j * ABFT_BLOCK + tid, lo, tt,
                                 &s_ncount[wave], s_notes[wave]);
              acc[j] = tt;
            }
          }
          // this wave's LDS reads have returned: the buffer may be refilled
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          if (lane == 0u) __hip_atomic_store(&s_done[wave], tile_no + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          lo = hi;
        }
      }
#pragma unroll
      for (int j = 0; j < RPT; j++) {
        const uint32_t o = out0 + (uint32_t)j * ABFT_BLOCK + tid;
        if (o < A.n_out) {
          y[o] = acc[j];
          if (FUSE) dsum += x[fuse.x_off + o] * acc[j];
        }
      }
      // cold: this wave's noted strangers go to the fix-up's queue (its own LDS list: no other wave touches it)
      const uint32_t notes = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_ncount[wave]);
      if (__builtin_expect(notes != 0u, 0)) {
        for (uint32_t k = lane; k < min(notes, PC_NOTES); k += 64u)
          coo_push_moved(A, ev, s_notes[wave][k].j, s_notes[wave][k].col, s_notes[wave][k].prod);
        if (notes > PC_NOTES && lane == 0u) push_event(ev, ABFT_EV_MOVED_OVERFLOW, PC_NOTES, 0, FMT_COO);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0u) s_ncount[wave] = 0u;
      }
    }
  }
  if (FUSE) {  // block_sum over the consumer waves (0-3: the lanes and order of the one-role kernel's partial)
    const double v = wave_sum(dsum);
    if (lane == 63u) s_w[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) fuse.partials[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
  }
  if (pace && wave == 4u && lane == 0u && my_slot < PACE_SLOTS) board[my_slot] = 0xffffffffu;
}

template <int MODE> static int coo_pc_occupancy() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spmv_coo_pc_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, true>, 512, 0) != hipSuccess || n < 1)
    n = 1;
  return n > 8 ? 8 : n;
}
int spmv_coo_pc_blocks_per_cu(int mode) {
  switch (mode) {
    case MODE_NONE: return coo_pc_occupancy<MODE_NONE>();
    case MODE_SED: return coo_pc_occupancy<MODE_SED>();
    case MODE_SEC7: return coo_pc_occupancy<MODE_SEC7>();
    case MODE_SEC8: return coo_pc_occupancy<MODE_SEC8>();
    default: return coo_pc_occupancy<MODE_SECDED>();
  }
}

template <int MODE>
static hipError_t launch_coo_pc_mode(const CooDev &A, const CsrPanels &P, const double *x, double *y, EventRing ev,
                                     const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s) {
  if (fuse)
    hipLaunchKernelGGL((spmv_coo_pc_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, true>), dim3(grid), dim3(512), 0, s, A, P, x, y, ev,
                       *fuse, c0, c1);
  else
    hipLaunchKernelGGL((spmv_coo_pc_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, false>), dim3(grid), dim3(512), 0, s, A, P, x, y, ev,
                       FuseOut{}, c0, c1);
  return hipGetLastError();
}

// (constraints mode keeps the one-role kernel: its checks need the successor table in the staging phase)
hipError_t launch_spmv_coo_pc(int mode, const CooDev &A, const CsrPanels &P, const double *x, double *y, EventRing ev,
                              const FuseOut *fuse, uint32_t grid, uint32_t chunk, hipStream_t s) {
  if (P.ngroups == 0) return hipSuccess;
  if (chunk == 0 || chunk > P.npanels) chunk = P.npanels;
  for (uint32_t c0 = 0; c0 < P.npanels; c0 += chunk) {
    const uint32_t c1 = c0 + chunk < P.npanels ? c0 + chunk : P.npanels;
    const FuseOut *f = c1 == P.npanels ? fuse : nullptr;
    hipError_t e;
    switch (mode) {
      case MODE_NONE: e = launch_coo_pc_mode<MODE_NONE>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SED: e = launch_coo_pc_mode<MODE_SED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC7: e = launch_coo_pc_mode<MODE_SEC7>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC8: e = launch_coo_pc_mode<MODE_SEC8>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SECDED: e = launch_coo_pc_mode<MODE_SECDED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int MODE>
static hipError_t launch_coo_panels_mode(const CooDev &A, const CsrPanels &P, const double *x, double *y,
                                         EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t c0,
                                         uint32_t c1, hipStream_t s) {
  if (fuse)
    hipLaunchKernelGGL((spmv_coo_panels_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, true>), dim3(grid), dim3(ABFT_BLOCK), 0, s, A,
                       P, x, y, ev, *fuse, c0, c1);
  else
    hipLaunchKernelGGL((spmv_coo_panels_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, false>), dim3(grid), dim3(ABFT_BLOCK), 0, s, A,
                       P, x, y, ev, FuseOut{}, c0, c1);
  return hipGetLastError();
}

hipError_t launch_spmv_coo_panels(int mode, const CooDev &A, const CsrPanels &P, const double *x, double *y,
                                  EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t chunk,
                                  hipStream_t s) {
  if (P.ngroups == 0) return hipSuccess;
  if (chunk == 0 || chunk > P.npanels) chunk = P.npanels;
  for (uint32_t c0 = 0; c0 < P.npanels; c0 += chunk) {
    const uint32_t c1 = c0 + chunk < P.npanels ? c0 + chunk : P.npanels;
    const FuseOut *f = c1 == P.npanels ? fuse : nullptr;
    hipError_t e;
    switch (mode) {
      case MODE_NONE: e = launch_coo_panels_mode<MODE_NONE>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_CONSTRAINTS: e = launch_coo_panels_mode<MODE_CONSTRAINTS>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SED: e = launch_coo_panels_mode<MODE_SED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC7: e = launch_coo_panels_mode<MODE_SEC7>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SEC8: e = launch_coo_panels_mode<MODE_SEC8>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      case MODE_SECDED: e = launch_coo_panels_mode<MODE_SECDED>(A, P, x, y, ev, f, grid, c0, c1, s); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int MODE> static int coo_panels_occupancy() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spmv_coo_panels_kernel<MODE, ABFT_CFG_COO_PANEL_EPT, true>, ABFT_BLOCK, 0) !=
          hipSuccess || n < 1)
    n = 1;
  return n > 8 ? 8 : n;
}
// workgroups of the COO panel kernel a CU holds at once (a paced launch needs all of its workgroups resident)
int spmv_coo_panels_blocks_per_cu(int mode) {
  switch (mode) {
    case MODE_NONE: return coo_panels_occupancy<MODE_NONE>();
    case MODE_CONSTRAINTS: return coo_panels_occupancy<MODE_CONSTRAINTS>();
    case MODE_SED: return coo_panels_occupancy<MODE_SED>();
    case MODE_SEC7: return coo_panels_occupancy<MODE_SEC7>();
    case MODE_SEC8: return coo_panels_occupancy<MODE_SEC8>();
    default: return coo_panels_occupancy<MODE_SECDED>();
  }
}

template <int MODE>
static hipError_t launch_spmv_coo_mode(const CooDev &A, const double *x, double *y, EventRing ev,
                                       const FuseOut *fuse, hipStream_t s) {
  if (fuse) {
    hipLaunchKernelGGL((spmv_coo_kernel<MODE, ABFT_COO_EPT, true>), dim3(A.nblk), dim3(ABFT_BLOCK), 0, s, A,
                       x, y, ev, *fuse);
  } else
    hipLaunchKernelGGL((spmv_coo_kernel<MODE, ABFT_COO_EPT, false>), dim3(A.nblk), dim3(ABFT_BLOCK), 0, s, A,
                       x, y, ev, FuseOut{});
  return hipGetLastError();
}

hipError_t launch_spmv_coo(int mode, const CooDev &A, const double *x, double *y, EventRing ev,
                           const FuseOut *fuse, hipStream_t s) {
  if (A.nblk == 0) return hipSuccess;
  switch (mode) {
    case MODE_NONE: return launch_spmv_coo_mode<MODE_NONE>(A, x, y, ev, fuse, s);
    case MODE_CONSTRAINTS: return launch_spmv_coo_mode<MODE_CONSTRAINTS>(A, x, y, ev, fuse, s);
    case MODE_SED: return launch_spmv_coo_mode<MODE_SED>(A, x, y, ev, fuse, s);
    case MODE_SEC7: return launch_spmv_coo_mode<MODE_SEC7>(A, x, y, ev, fuse, s);
    case MODE_SEC8: return launch_spmv_coo_mode<MODE_SEC8>(A, x, y, ev, fuse, s);
    case MODE_SECDED: return launch_spmv_coo_mode<MODE_SECDED>(A, x, y, ev, fuse, s);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------ sweep-layout SpMV --

// Sweep-layout SpMV (CSR; see SweepLayout).  Stages a segment tile by tile through LDS with
// the same branch-free load phase as the streaming kernel (ECC in registers, cold path out
// of line); each thread then adds the staged products of its rows, in element order, onto
// its running sums -- a row's additions happen in the caller's order (panels ascend, and
// inside a panel its elements keep their order), so y stays bit-identical to the reference
// (CSR/CPUContext.cpp:115-133 and variants).  RPT rows per thread: 256 * RPT rows per
// workgroup, chosen at create time so that all groups are resident at once.
template <int MODE, int RPT>
__global__ __launch_bounds__(ABFT_BLOCK, (RPT == 16 || MODE == MODE_CONSTRAINTS) ? 4 : 5) void spmv_sweep_kernel(CsrDev A, SweepLayout L,
                                                                const double *__restrict__ x, double *__restrict__ y,
                                                                EventRing ev, FuseOut fuse, bool fused, uint32_t c0,
                                                                uint32_t c1) {
  constexpr int EPT = RPT <= 4 ? 4 : ABFT_CFG_SWEEP_EPT;  // small groups have small segments: smaller tiles
  constexpr uint32_t TILE = ABFT_BLOCK * EPT, GROUP = 256u * RPT;
  // the next tile's streaming loads issued behind this tile's gathers, one tile ahead in registers
  constexpr bool PF = (ABFT_CFG_SWEEP_PREFETCH >> (RPT == 16 ? 1 : 0)) & 1;
  // two product buffers: a wave that has summed tile t goes straight on to stage tile t + 1 into
  // the other buffer -- one workgroup barrier per tile (behind the staging) instead of two, and the
  // waves of a workgroup may be a phase apart (everyone has left tile t - 1's sums, which read the
  // buffer now being written, before anyone passed tile t's barrier)
  // (where 5 workgroups per CU are wanted -- every RPT but 16 -- two 16 KB buffers would not fit
  // beside each other five times: one buffer, two barriers)
  // (constraints mode stages the columns too: one buffer set.  Measured, round 3, config 4, ms per 100 iterations
  // against 72.5 in `none`: as is 103-104; 4 elements per thread and tile, two buffer sets, no scratch: 109;
  // 4 rows per thread: 102; pacing lag 0 / 3: 104 / 107; the loop and its event sites out of line behind a
  // straight-line path for one- and two-element cells: 117.  rocprofv3: 147 M scalar and 178 M vector
  // instructions per SpMV against 36 M and 98 M in `none` -- the per-cell control flow, not memory.)
  constexpr bool TWO = (RPT == 16 || EPT <= 4) && MODE != MODE_CONSTRAINTS;
  __shared__ __attribute__((aligned(16))) double s_buf[TWO ? 2 : 1][TILE];
  // constraints mode: the staged columns too (the checks of reference CSR/CPUContext.cpp:186-200 run in
  // the summing phase, element by element in the row's order)
  constexpr bool CONS = MODE == MODE_CONSTRAINTS;
  __shared__ __attribute__((aligned(16))) uint32_t s_colbuf[CONS ? (TWO ? 2 : 1) : 1][CONS ? TILE : 2];
  uint32_t par = 0;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nsteps = c1 - c0;
  const uint32_t nrounds = (L.ngroups + gridDim.x - 1u) / gridDim.x;
  const bool pace = L.lag != 0u;
  uint32_t *board = nullptr;       // this XCD's progress board
  uint32_t my_slot = 0xffffffffu;  // wave 0: where this workgroup publishes (only lane 0 stores)
  if (pace) {
    // slot = blockIdx / 8: workgroups are dealt to the XCDs round-robin, so the slots of one board
    // are distinct (were two workgroups of an XCD ever to share one, the board would show the later
    // writer: pacing a little less exact, nothing else).  No registration, no exit ticket: the two
    // agent-scope atomics per workgroup those took cost more than the pacing gained.
    board = L.pace + xcc_id() * PACE_SLOTS;
    if (wave == 0u) {
      my_slot = blockIdx.x >> 3;
      if (lane == 0u && my_slot < PACE_SLOTS) board[my_slot] = 0u;
    }
  }
  double dsum = 0.0;
  BoardView seen{~0ull, ~0ull};    // wave 0: the board as loaded one step ago
  bool have_seen = false, gave_up = false;
  uint32_t dbg_spins = 0, dbg_waits = 0;
#ifdef ABFT_DBG_STAMPS
  unsigned long long dbg_t[6] = {0, 0, 0, 0, 0, 0};
  STAMP(t_begin);
#endif
  for (uint32_t round = 0; round < nrounds; round++) {
    const uint32_t g = blockIdx.x + round * gridDim.x;
    if (g >= L.ngroups) {  // the last round may be short: nobody of this XCD has to wait for us
      if (pace && threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = 0xffffffffu;
      continue;
    }
    const uint32_t out0 = g * GROUP + wave * (64u * RPT) + lane;  // this thread's rows: out0 + 64 j
    double acc[RPT];
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t o = out0 + 64u * (uint32_t)j;
      acc[j] = (c0 > 0 && o < A.n_out) ? y[o] : 0.0;
    }
    // constraints mode, per row of this thread: the column of its last element so far PLUS ONE (a row's
    // elements sit in several panels; the order check between the last one of a panel and the first of the
    // next needs it).  0: no element yet (every column passes `col >= 0`); ~0: the row has failed a check
    // (no column passes `col >= ~0`, which sends every later element of the row down the cold path, where
    // it is dropped).
    uint32_t cons_lp1[CONS ? RPT : 1];
    if (CONS) {
#pragma unroll
      for (int j = 0; j < RPT; j++) {
        cons_lp1[j] = 0u;
        const uint32_t row = out0 + 64u * (uint32_t)j;
        if (row < A.n_out) {  // the two row-pointer checks (reference CSR/CPUContext.cpp:173-182)
          const uint32_t rs = A.rowptr[row], re = A.rowptr[row + 1];
          if (re > A.nnz) { push_event(ev, ABFT_EV_ROW_SIZE, row, row, FMT_CSR); cons_lp1[j] = 0xffffffffu; }
          else if (re < rs) { push_event(ev, ABFT_EV_ROW_ORDER, row, row, FMT_CSR); cons_lp1[j] = 0xffffffffu; }
        }
      }
    }
    const uint32_t *wb = L.wbase + 4u * (size_t)g * L.npanels;
    CsrTileRegs<EPT> tr_cur, tr_nxt;
    uint32_t pf_base = 0xffffffffu;  // PF: base of the tile whose loads are in tr_cur
    for (uint32_t c = c0; c < c1; c++) {
      const uint32_t step = round * nsteps + (c - c0);
      const uint32_t e0 = wb[4u * c], e1 = wb[4u * c + 4u];
      if (e0 != e1) {  // uniform
        STAMP(tA);
        // ---- this thread's RPT counts (one byte each) -> element ranges of its rows ----
        uint32_t cw[RPT >= 4 ? RPT / 4 : 1];
        {
          const uint8_t *cp = L.counts + ((size_t)(g * L.npanels + c) * 256u + threadIdx.x) * RPT;
          if (RPT == 2) cw[0] = *reinterpret_cast<const uint16_t *>(cp);
          else {
#pragma unroll
            for (int k = 0; k < RPT / 4; k++)
#if ABFT_CFG_SWEEP_COUNTS_NT  // the counts are read once per SpMV, like the elements: keep them out of the way of x in L2
              cw[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(cp) + k);
#else
              cw[k] = reinterpret_cast<const uint32_t *>(cp)[k];
#endif
          }
        }
        uint32_t start[RPT];
        uint32_t run = wb[4u * c + wave];  // wave-uniform
#pragma unroll
        for (int m = 0; m < RPT / 2; m++) {  // two counts per scan, in 16-bit halves (64 * 255 < 65536)
          const uint32_t b0 = (cw[m / 2] >> (16 * (m & 1))) & 0xffu, b1 = (cw[m / 2] >> (16 * (m & 1) + 8)) & 0xffu;
          const uint32_t inc = wave_scan_u32(b0 | (b1 << 16));
          const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
          start[2 * m] = run + (inc & 0xffffu) - b0;
          run += tot & 0xffffu;
          start[2 * m + 1] = run + (inc >> 16) - b1;
          run += tot >> 16;
        }
        STAMP(tB);
        STAMP_ADD(0, tA, tB);
        if (pace && wave == 0u) {
          // before gathering from panel `step`: the slowest workgroup of this XCD must have
          // completed step - lag + 1 steps (all of them then sit within `lag` panels).  The
          // board was loaded one step ago -- that load's latency ran beside the step's work --
          // and only a minimum still short then sends this wave polling (bounded).
          if (step >= L.lag && !gave_up) {
            const uint32_t need = step + 1u - L.lag;
            uint32_t m = have_seen ? board_min(seen) : 0u;
            if (m < need) {
              dbg_waits++;
              int it = 0;
              for (; it < 1024 && m < need; it++) {
                __builtin_amdgcn_s_sleep(4);
                m = board_min(board_load(board, lane));
                dbg_spins++;
              }
              // ~1 ms and still short: a workgroup of this XCD is not running (CUs taken by another
              // stream's kernels?) -- stop pacing for the rest of this launch rather than stall again
              if (it == 1024) gave_up = true;
            }
          }
          seen = board_load(board, lane);
          have_seen = true;
        }
        STAMP(tC);
        STAMP_ADD(1, tB, tC);
        for (uint32_t lo = e0; lo < e1;) {
          STAMP(tD0);
          const uint32_t b = lo & ~1u;
          const uint32_t hi = min(e1, b + TILE);
          double *s_prod = s_buf[TWO ? par : 0u];
          uint32_t *s_col = s_colbuf[CONS && TWO ? par : 0u];
          par ^= 1u;
          if (!TWO) __syncthreads();
          if (PF) {
            if (pf_base != b) csr_issue_loads<EPT>(A, b, hi, tr_cur);  // nothing ahead yet: the group's first tile
            // the tile after this one: the rest of the segment, or the head of the next non-empty one
            uint32_t nlo = hi, ne1 = e1;
            bool more = hi < e1;
            if (!more)
              for (uint32_t cn = c + 1u; cn < c1 && !more; cn++) {
                nlo = wb[4u * cn]; ne1 = wb[4u * cn + 4u];
                more = nlo != ne1;
              }
            const uint32_t nb = more ? (nlo & ~1u) : b, nhi = more ? min(ne1, nb + TILE) : b;
            csr_consume<MODE, EPT>(A, x, ev, b, lo, hi, tr_cur, s_prod, s_col, true, nb, nhi, tr_nxt);
            tr_cur = tr_nxt;
            pf_base = more ? nb : 0xffffffffu;
          } else {
            csr_stage<MODE, EPT>(A, x, ev, b, lo, hi, s_prod, s_col);
          }
          STAMP(tD);
          STAMP_ADD(2, tD0, tD);
          __syncthreads();
          STAMP(tE);
          STAMP_ADD(3, tD, tE);
#ifdef ABFT_DBG_NOPHASE2  // timing-only build: wrong results
          if (threadIdx.x == 1023u)
#endif
#pragma unroll
          for (int j = 0; j < RPT; j++) {
            const uint32_t cj = (cw[j / 4] >> (8 * (j & 3))) & 0xffu;
            const uint32_t a0 = max(start[j], lo), a1 = min(start[j] + cj, hi);
            if (a0 < a1) {
              double t = acc[j];
              if (CONS) {
                // the row's elements of this panel and tile, in the row's order: column inside the vector,
                // column above its predecessor's (reference CSR/CPUContext.cpp:186-200; the predecessor of a
                // panel's first element is the last element of the row in an earlier panel).  One element is
                // the common case and gets a straight-line path: two compares, one add.
                uint32_t lp1 = cons_lp1[j];
                const uint32_t c0 = s_col[a0 - b];
                if (__builtin_expect(a1 - a0 == 1u && c0 >= lp1 && c0 < A.n_in, 1)) {
                  t += s_prod[a0 - b];
                  lp1 = c0 + 1u;
                } else if (lp1 != 0xffffffffu) {
                  const uint32_t row = out0 + 64u * (uint32_t)j;
                  for (uint32_t i = a0; i < a1; i++) {
                    const uint32_t col = s_col[i - b];
                    if (col < lp1) {  // reported at the predecessor: the caller's element before this one
                      push_event(ev, ABFT_EV_COL_ORDER, event_index_of_orig(A, A.orig_index[i] - 1u), row, FMT_CSR);
                      lp1 = 0xffffffffu;
                      break;
                    }
                    if (col >= A.n_in) {
                      push_event(ev, ABFT_EV_COL_SIZE, event_index(A, i), row, FMT_CSR);
                      lp1 = 0xffffffffu;
                      break;
                    }
                    t += s_prod[i - b];
                    lp1 = col + 1u;
                  }
                }
                cons_lp1[j] = lp1;
              } else {
                csr_row_sum<MODE, ABFT_CFG_SWEEP_SHORT_SUMS>(A, ev, b, a0, a1, a1, s_prod, s_col, t);
              }
              acc[j] = t;
            }
          }
          STAMP(tF);
          STAMP_ADD(4, tE, tF);
          lo = hi;
        }
      }
      if (pace && threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = step + 1u;  // plain store: into this XCD's L2
    }
    // (the fused product's operands first, all in flight together: read inside the loop below hipcc waits for each
    // before it issues the next -- RPT trips to memory in a row at the end of every workgroup)
    double xo[RPT];
#pragma unroll
    for (int j = 0; j < RPT; j++) xo[j] = fused ? x[fuse.x_off + min(out0 + 64u * (uint32_t)j, A.n_out - 1u)] : 0.0;
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const uint32_t o = out0 + 64u * (uint32_t)j;
      if (o < A.n_out && !(CONS && cons_lp1[CONS ? j : 0] == 0xffffffffu)) {  // (a row that failed a check is left alone, as in the streaming kernel)
        y[o] = acc[j];
        if (fused) dsum += xo[j] * acc[j];
      }
    }
  }
  if (fused) fused_dot_finish(dsum, fuse, blockIdx.x);
  if (pace) {
    if (threadIdx.x == 0 && L.debug) {
      atomicAdd(L.debug, dbg_spins);
      atomicAdd(L.debug + 1, dbg_waits);
      atomicAdd(L.debug + 2, 1u);
#ifdef ABFT_DBG_STAMPS
      STAMP(t_end);
      dbg_t[5] = t_end - t_begin;
      for (int k = 0; k < 6; k++) atomicAdd(reinterpret_cast<unsigned long long *>(L.debug + 4) + k, dbg_t[k]);
      if (L.debug_wg) {  // per workgroup, summed over launches: where the SLOW workgroups of an XCD lose their time
        uint32_t hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned long long *w = L.debug_wg + 4u * blockIdx.x;
        w[0] += dbg_t[5]; w[1] += dbg_t[1]; w[2] += dbg_t[2];
        w[3] = ((unsigned long long)xcc_id() << 32) | hw;
      }
#endif
    }
    // done: never holds anyone back, and the board is clean for the next launch
    if (threadIdx.x == 0 && my_slot < PACE_SLOTS) board[my_slot] = 0xffffffffu;
  }
}

template <int MODE, int RPT>
static hipError_t launch_sweep_inst(const CsrDev &A, const SweepLayout &L, const double *x, double *y, EventRing ev,
                                    const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s) {
  hipLaunchKernelGGL((spmv_sweep_kernel<MODE, RPT>), dim3(grid), dim3(ABFT_BLOCK), 0, s, A, L, x, y, ev,
                     fuse ? *fuse : FuseOut{}, fuse != nullptr, c0, c1);
  return hipGetLastError();
}

template <int MODE, int RPT> static int sweep_occupancy_inst() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spmv_sweep_kernel<MODE, RPT>, ABFT_BLOCK, 0) != hipSuccess || n < 1)
    n = 1;
  return n > 8 ? 8 : n;
}

// one switch for both uses: OP(MODE, RPT)
#define ABFT_SWEEP_DISPATCH(OP)                                                                    \
  switch (mode * 100 + rpt) {                                                                      \
    ABFT_SWEEP_MODE(OP, MODE_NONE) ABFT_SWEEP_MODE(OP, MODE_CONSTRAINTS) ABFT_SWEEP_MODE(OP, MODE_SED)  \
    ABFT_SWEEP_MODE(OP, MODE_SEC7)                                                                 \
    ABFT_SWEEP_MODE(OP, MODE_SEC8) ABFT_SWEEP_MODE(OP, MODE_SECDED)                                \
    default: break;                                                                                \
  }
#define ABFT_SWEEP_MODE(OP, M)                 \
  case M * 100 + 2: OP(M, 2); break;           \
  case M * 100 + 4: OP(M, 4); break;           \
  case M * 100 + 8: OP(M, 8); break;           \
  case M * 100 + 16: OP(M, 16); break;

hipError_t launch_spmv_sweep(int mode, int rpt, const CsrDev &A, const SweepLayout &L, const double *x, double *y,
                             EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s) {
  if (L.ngroups == 0 || c0 >= c1) return hipSuccess;
  if (c1 > L.npanels || grid == 0) return hipErrorInvalidValue;
  hipError_t e = hipErrorInvalidValue;
#define ABFT_OP(M, R) e = launch_sweep_inst<M, R>(A, L, x, y, ev, fuse, grid, c0, c1, s)
  ABFT_SWEEP_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return e;
}

int spmv_sweep_blocks_per_cu(int mode, int rpt) {
  int n = 1;
#define ABFT_OP(M, R) n = sweep_occupancy_inst<M, R>()
  ABFT_SWEEP_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return n;
}

// ------------------------------------------------------------ slice-layout SpMV --

// A wave-uniform word through the scalar cache.  hipcc only emits s_load for memory it can prove
// nobody writes during the kernel; for a table reached through a struct member it falls back to a
// vector load, whose s_waitcnt vmcnt(0) would drain every streaming load and gather in flight.
__device__ __forceinline__ uint32_t scalar_load_u32(const uint32_t *p) {
  uint32_t v;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
  return v;
}

// DPP moves across the whole wave (GFX9: wave_shr:1 / wave_shl:1); a lane without a source keeps `old`
__device__ __forceinline__ uint32_t wave_shr1_u32(uint32_t v, uint32_t old) {  // lane i <- lane i - 1
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_shl1_u32(uint32_t v, uint32_t old) {  // lane i <- lane i + 1
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xf, 0xf, false);
}
__device__ __forceinline__ double wave_shl1_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// One chunk of 64 stored elements (one per lane, in storage order) added onto the wave's row
// sums in LDS: lane i holds the product `p` of an element of local row r - 1 (r == 0: no element).
// Inside one panel's part of a slice rows ascend, so the elements of one row are a run of lanes; the
// run's first lane reads the row's sum, adds its own product and then its followers' in lane order
// (the first follower unconditionally -- most chunks hold a pair -- longer runs in a loop of one DPP
// shift per step) and writes the sum back.  A row that goes on in the next chunk is picked up there
// by its first lane: the wave's LDS operations execute in order.  RANGED: only lanes [lo, hi) -- the
// caller never folds elements of two panels at once: the same row may come again behind a panel
// boundary, and two runs of one row in one call would both start from the old sum.
// `accm1` = the wave's sums - 1 (so that r indexes it directly).
template <bool RANGED>
__device__ __forceinline__ void slice_fold(double *accm1, uint32_t r, double p, uint32_t lo = 0u, uint32_t hi = 64u) {
  if (RANGED) {
    const uint32_t lane = threadIdx.x & 63u;
    r = (lane >= lo && lane < hi) ? r : 0u;
  }
  const uint32_t prev = wave_shr1_u32(r, 0u);
  const bool head = r != 0u && r != prev;
  double a = 0.0;
  if (head) a = accm1[r];
  a += p;
  uint32_t rq = wave_shl1_u32(r, 0u);  // row and product of lane i + 1
  double q = wave_shl1_f64(p);
  bool still = head && rq == r;
  if (still) a += q;
  rq = wave_shl1_u32(rq, 0u);
  still = still && rq == r;
  while (__builtin_amdgcn_ballot_w64(still) != 0ull) {  // runs of three and more: rare
    q = wave_shl1_f64(wave_shl1_f64(p));  // (recomputed here, off the common path)
    uint32_t rr = rq;
    for (;;) {
      if (still) a += q;
      rr = wave_shl1_u32(rr, 0u);
      q = wave_shl1_f64(q);
      still = still && rr == r;
      if (__builtin_amdgcn_ballot_w64(still) == 0ull) break;
    }
  }
  if (head) accm1[r] = a;
}

// Slice-layout SpMV (CSR; see SliceLayout): every wave owns slices s, s + (waves of the grid), ...
// and streams each slice's run of elements K chunks of 64 at a time -- streaming loads of value,
// column and row id, ECC in registers (cold path out of line, as everywhere), gather, multiply,
// ordered fold into the wave's own row sums in LDS.  No barrier inside the sweep, no atomics, no
// per-(row, panel) bookkeeping.  Reference order of additions: CSR/CPUContext.cpp:115-133 and the
// ABFT variants.
//
// What bounds this kernel is the number of instructions issued per element (the first version spent
// 150 vector and 80 scalar instructions per chunk and ran at 80 % issue occupancy), so:
//   * every load is a buffer load: the address is base (SGPRs) + a 32-bit byte offset, and an offset
//     past the end returns 0 -- no 64-bit address arithmetic, no clamping, no validity flags: a lane
//     past the slice's end loads row id 0 = "no element", a column outside the gathered vector
//     gathers 0.0 (the documented behaviour);
//   * the chunks of one step share their offset registers (instruction offsets k * 512 / 256 / 128).
// A wave is on its own here (no sibling fills its memory waits by construction of a tile), so the
// loop is software-pipelined three deep: while the products of step i are folded, the gathers of
// step i + 1 and the streaming loads of step i + 2 are in flight.  Branch-free: steps past the
// slice's end load zeros and fold nothing.
//
// Pacing (speed only, as in the sweep kernel: the per-XCD progress board, plain stores, one
// L1-bypassing load of the board per panel, every wait bounded).  The unit that publishes is the
// workgroup: every wave notes the panel its gathers have reached in LDS, wave 0 -- when its own
// changes, every few steps, in its own waits and, once its slices are done, until the other three are
// done too -- stores the minimum of the four on the board when it has changed (one writer per slot:
// monotone).  A wave whose gathers enter panel step t first needs every workgroup of its XCD to have
// completed t - lag steps: the waves of an XCD gather from at most lag + 1 consecutive panels.
template <int K> struct SliceLoads { u32x2 v[K]; uint32_t c[K], r[K]; };
template <int K> struct SliceProds { double v[K], xv[K]; uint32_t r[K]; };

constexpr int BUF_NT = 2;                  // aux of a buffer load: non-temporal
constexpr uint32_t BUF_WORD3 = 0x00020000u;  // untyped 32-bit data, no swizzle, no add-tid

// streaming loads of the step at `pos` (element index inside the slice, this lane's, chunk 0)
template <int K>
__device__ __forceinline__ void slice_issue_loads(__amdgpu_buffer_rsrc_t bv, __amdgpu_buffer_rsrc_t bc,
                                                  __amdgpu_buffer_rsrc_t br, uint32_t pos, SliceLoads<K> &t) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    t.v[k] = __builtin_amdgcn_raw_buffer_load_b64(bv, (pos << 3) + 512 * k, 0, BUF_NT);
    t.c[k] = __builtin_amdgcn_raw_buffer_load_b32(bc, (pos << 2) + 256 * k, 0, BUF_NT);
    t.r[k] = __builtin_amdgcn_raw_buffer_load_b16(br, (pos << 1) + 128 * k, 0, BUF_NT);
  }
}

// ECC check of the loaded elements of a step, their gathers issued; products are formed at the fold.
// `first` = stored position of this lane's chunk-0 element (cold path only).
template <int MODE, int K>
__device__ __forceinline__ void slice_consume(const CsrDev &A, __amdgpu_buffer_rsrc_t bx, const EventRing &ev,
                                              uint32_t first, const SliceLoads<K> &t, SliceProds<K> &o) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    uint32_t w[3] = {t.v[k].x, t.v[k].y, t.c[k]};
    bool fatal = false;
    if (MODE >= MODE_SED) {
      // (a lane past the slice's end holds three zero words: a clean codeword in every mode)
      if (__builtin_expect(ecc_suspect<FMT_CSR, MODE>(w) != 0, 0)) {
        const uint32_t i = first + 64u * (uint32_t)k;
        EccWords<FMT_CSR> ew;
        ew.w[0] = w[0]; ew.w[1] = w[1]; ew.w[2] = w[2]; ew.rc = 0;
        ew = ecc_cold<FMT_CSR, MODE>(ew, event_index(A, i), ev);
        w[0] = ew.w[0]; w[1] = ew.w[1]; w[2] = ew.w[2];
        if (ew.rc > 0) {  // reference CSR/CPUContext.cpp:275-276, 333-334, 389-390
          A.vals[i] = as_double(w[0], w[1]);
          A.cols[i] = w[2];
        } else {
          fatal = true;  // the reference never uses this element
        }
      }
      w[2] &= ABFT_COLMASK;
    }
    // the gather: an index outside the vector reads 0.0 (bounds-checked by the buffer); 2^29 and more
    // would wrap the byte offset, so they are pinned to one that is out of range for any vector
#ifdef ABFT_DBG_NOGATHER  // timing-only build: wrong results
    o.xv[k] = (double)w[2];
#else
    const u32x2 g = __builtin_amdgcn_raw_buffer_load_b64(bx, min(w[2], 0x1fffffffu) << 3, 0, 0);
    o.xv[k] = as_double(g.x, g.y);
#endif
    // (no use of xv here: the gather stays in flight until the fold)
    o.v[k] = fatal ? 0.0 : as_double(w[0], w[1]);
    o.r[k] = t.r[k];
  }
}

template <int MODE, int K>
__global__ __launch_bounds__(ABFT_BLOCK, ABFT_CFG_SLICE_WAVES) void spmv_slice_kernel(
    CsrDev A, SliceLayout L, const double *__restrict__ x, double *__restrict__ y, EventRing ev, FuseOut fuse,
    bool fused, uint32_t c0, uint32_t c1) {
  extern __shared__ __attribute__((aligned(16))) double s_rows[];  // 4 waves x 2^rows_log2 row sums
  __shared__ uint32_t s_prog[4];  // panel steps each wave has completed
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t R = 1u << L.rows_log2;
  double *acc = s_rows + (size_t)wave * R;
  const uint32_t nwaves = gridDim.x * 4u, nsteps = c1 - c0;
  const uint32_t nrounds = (L.nslices + nwaves - 1u) / nwaves;
  const uint32_t slot = blockIdx.x >> 3;  // workgroups are dealt to the XCDs round-robin: distinct slots per board
  const bool pace = L.lag != 0u && slot < PACE_SLOTS;
  uint32_t *board = pace ? L.pace + xcc_id() * PACE_SLOTS : nullptr;
  uint32_t last_pub = 0u, last_done = 0u, since_pub = 0u;
  BoardView seen{~0ull, ~0ull};
  bool have_seen = false, gave_up = false;
  if (pace) {
    if (lane == 0u) s_prog[wave] = 0u;
    if (threadIdx.x == 0u) board[slot] = 0u;
    __syncthreads();
  }
  // wave 0: the workgroup's progress = the slowest of its four waves, stored when it has changed
  auto publish = [&]() {
    // (atomic: re-read every time, never cached in a register across the loops below)
    const uint32_t m = min(min(__hip_atomic_load(&s_prog[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP),
                               __hip_atomic_load(&s_prog[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)),
                           min(__hip_atomic_load(&s_prog[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP),
                               __hip_atomic_load(&s_prog[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)));
    if (m != last_pub) {
      last_pub = m;
      if (lane == 0u) board[slot] = m;  // plain store: into this XCD's L2
    }
    since_pub = 0u;
    return m;
  };
  constexpr uint32_t STEP = 64u * K;
  const __amdgpu_buffer_rsrc_t bx = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(x), 0, (int)(A.n_in * 8u), BUF_WORD3);
  double dsum = 0.0;
  for (uint32_t round = 0; round < nrounds; round++) {
    const uint32_t s = round * nwaves + blockIdx.x * 4u + wave;
    if (s >= L.nslices) break;  // (uniform per wave; the tail below reports this wave as done)
    const uint32_t row0 = s << L.rows_log2;
    for (uint32_t i = lane; i < R; i += 64u) {
      const uint32_t row = row0 + i;
      acc[i] = (c0 > 0u && row < A.n_out) ? y[row] : 0.0;  // a later panel range resumes from y (exact)
    }
    const uint32_t *sb = L.sub + (size_t)s * (L.npanels + 1u);
    const uint32_t e0 = scalar_load_u32(sb + c0), e1 = scalar_load_u32(sb + c1);  // wave-uniform
    const uint32_t len = e1 - e0;
    // this slice's run of each array as a buffer: offsets count from e0, anything past e1 reads 0
    const __amdgpu_buffer_rsrc_t bv = __builtin_amdgcn_make_buffer_rsrc(A.vals + e0, 0, (int)(len * 8u), BUF_WORD3);
    const __amdgpu_buffer_rsrc_t bc = __builtin_amdgcn_make_buffer_rsrc(A.cols + e0, 0, (int)(len * 4u), BUF_WORD3);
    const __amdgpu_buffer_rsrc_t br =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(L.rid) + e0, 0, (int)(len * 2u), BUF_WORD3);
    uint32_t pc = c0, pend = scalar_load_u32(sb + c0 + 1u) - e0;  // gather cursor: panel `pc` ends at slice position pend
    uint32_t cur = c0, nb = pend;                                   // fold cursor, one step behind
    // before the gathers of step [e, e + STEP) go out: progress, and the pacing check when they enter a new panel
    auto pace_step = [&](uint32_t e) {
      const uint32_t done = round * nsteps + (pc - c0);  // every panel before the previous step's last is behind this wave
      const uint32_t last = min(e + STEP, len) - 1u;
      bool entered = false;
      while (pend <= last && pc + 1u < c1) { pc++; pend = scalar_load_u32(sb + pc + 1u) - e0; entered = true; }
      if (done != last_done) {
        last_done = done;
        if (lane == 0u) __hip_atomic_store(&s_prog[wave], done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        since_pub = 8u;
      }
      if (wave == 0u && ++since_pub >= 8u) publish();
      if (entered && !gave_up) {
        const uint32_t step = round * nsteps + (pc - c0);
        if (step > L.lag) {
          // (the step that enters panel `step` also ends panel step - 1, so this wave itself has
          // completed `done` < step steps: it never waits for more than that)
          const uint32_t need = min(step - L.lag, done);
          uint32_t m = have_seen ? board_min(seen) : 0u;
          if (m < need) {
            int it = 0;
            for (; it < 1024 && m < need; it++) {
              __builtin_amdgcn_s_sleep(4);
              if (wave == 0u) publish();
              m = board_min(board_load(board, lane));
            }
            if (it == 1024) gave_up = true;  // ~1 ms: a workgroup of this XCD is not running -- stop pacing
          }
        }
        seen = board_load(board, lane);  // for the next panel: its latency runs beside this panel's work
        have_seen = true;
      }
    };
    SliceLoads<K> ld;
    SliceProds<K> p0, p1;
    double *accm1 = acc - 1;
    if (len) {
      slice_issue_loads<K>(bv, bc, br, lane, ld);
      if (pace) pace_step(0u);
      slice_consume<MODE, K>(A, bx, ev, e0 + lane, ld, p0);
      slice_issue_loads<K>(bv, bc, br, STEP + lane, ld);
    }
    for (uint32_t e = 0; e < len; e += STEP) {  // e: position inside the slice
      // in flight here: the gathers of step e (p0), the streaming loads of step e + STEP (ld)
      if (pace && e + STEP < len) pace_step(e + STEP);
      slice_consume<MODE, K>(A, bx, ev, e0 + e + STEP + lane, ld, p1);  // (past the end: zeros, nothing to fold)
      slice_issue_loads<K>(bv, bc, br, e + 2u * STEP + lane, ld);
#pragma unroll
      for (int k = 0; k < K; k++) {
        const uint32_t b = e + 64u * (uint32_t)k;  // slice position of lane 0's element
        const double p = p0.v[k] * p0.xv[k];
        if (nb >= b + 64u || cur + 1u >= c1) {  // (uniform) the whole chunk lies in one panel: nearly always
          slice_fold<false>(accm1, p0.r[k], p);
        } else {
          // one fold per panel the chunk holds elements of
          for (uint32_t lo = 0u; b + lo < len;) {
            while (nb <= b + lo && cur + 1u < c1) { cur++; nb = scalar_load_u32(sb + cur + 1u) - e0; }
            const uint32_t hi = nb - b < 64u ? nb - b : 64u;
            slice_fold<true>(accm1, p0.r[k], p, lo, hi);
            if (hi >= 64u) break;
            lo = hi;
          }
        }
      }
      p0 = p1;
    }
    for (uint32_t i = lane; i < R; i += 64u) {
      const uint32_t row = row0 + i;
      if (row < A.n_out) {
        const double a = acc[i];
        y[row] = a;
        if (fused) dsum += x[fuse.x_off + row] * a;
      }
    }
  }
  if (pace) {
    // this wave is done with every round; wave 0 goes on publishing until its three neighbours are too,
    // then leaves the slot at "nobody here" (clean for the next launch, and never holding anyone back)
    if (lane == 0u) __hip_atomic_store(&s_prog[wave], 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (wave == 0u) {
      for (int it = 0; it < (1 << 20) && publish() != 0xffffffffu; it++) __builtin_amdgcn_s_sleep(8);
      if (lane == 0u) board[slot] = 0xffffffffu;
    }
  }
  if (fused) fused_dot_finish(dsum, fuse, blockIdx.x);
}

template <int MODE>
static hipError_t launch_slice_inst(const CsrDev &A, const SliceLayout &L, const double *x, double *y, EventRing ev,
                                    const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s) {
  const size_t lds = (size_t)4 * sizeof(double) << L.rows_log2;
  hipLaunchKernelGGL((spmv_slice_kernel<MODE, ABFT_CFG_SLICE_K>), dim3(grid), dim3(ABFT_BLOCK), lds, s, A, L, x, y, ev,
                     fuse ? *fuse : FuseOut{}, fuse != nullptr, c0, c1);
  return hipGetLastError();
}

hipError_t launch_spmv_slice(int mode, const CsrDev &A, const SliceLayout &L, const double *x, double *y, EventRing ev,
                             const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s) {
  if (L.nslices == 0 || c0 >= c1) return hipSuccess;
  if (c1 > L.npanels || grid == 0 || L.rows_log2 > 11u) return hipErrorInvalidValue;
  switch (mode) {
    case MODE_NONE: return launch_slice_inst<MODE_NONE>(A, L, x, y, ev, fuse, grid, c0, c1, s);
    case MODE_SED: return launch_slice_inst<MODE_SED>(A, L, x, y, ev, fuse, grid, c0, c1, s);
    case MODE_SEC7: return launch_slice_inst<MODE_SEC7>(A, L, x, y, ev, fuse, grid, c0, c1, s);
    case MODE_SEC8: return launch_slice_inst<MODE_SEC8>(A, L, x, y, ev, fuse, grid, c0, c1, s);
    case MODE_SECDED: return launch_slice_inst<MODE_SECDED>(A, L, x, y, ev, fuse, grid, c0, c1, s);
    default: return hipErrorInvalidValue;
  }
}

template <int MODE> static int slice_occupancy_inst(size_t lds) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spmv_slice_kernel<MODE, ABFT_CFG_SLICE_K>, ABFT_BLOCK, lds) !=
          hipSuccess || n < 1)
    n = 1;
  return n > 8 ? 8 : n;
}

int spmv_slice_blocks_per_cu(int mode, uint32_t rows_log2) {
  const size_t lds = (size_t)4 * sizeof(double) << rows_log2;
  switch (mode) {
    case MODE_NONE: return slice_occupancy_inst<MODE_NONE>(lds);
    case MODE_SED: return slice_occupancy_inst<MODE_SED>(lds);
    case MODE_SEC7: return slice_occupancy_inst<MODE_SEC7>(lds);
    case MODE_SEC8: return slice_occupancy_inst<MODE_SEC8>(lds);
    default: return slice_occupancy_inst<MODE_SECDED>(lds);
  }
}

// ------------------------------------------------- COO: corrupted-column fix-up --

// Launched behind every COO SpMV (one workgroup; returns at once when the SpMV queued
// nothing, which is every launch on clean data).  The SpMV left each moved product out of
// the sum of the group it is stored in -- that output is already what the reference
// computes -- and queued {caller's index, new column, product}.  Here every output that
// RECEIVES products is rebuilt from 0.0 as the reference's serial loop builds it
// (COO/CPUContext.cpp:111-120): its own elements that still name it, re-multiplied from
// the (repaired) stored words, merged by caller's index with the queued products.
// Stored order inside a group is the caller's order in both layouts, so the merge is a
// two-way merge.  A fused vec.result product is corrected through partial 0.
__device__ __forceinline__ void fixup_range(const CooDev &A, const FixLayout &F, uint32_t c, uint32_t rg, uint32_t &lo,
                                            uint32_t &hi) {
  if (F.kind == 0) { lo = A.grp_ptr[c]; hi = A.grp_ptr[c + 1]; return; }
  const uint32_t seg = (c / ABFT_PANEL_ROWS) * F.P.npanels + rg;
  const uint32_t e0 = F.P.seg_base[seg];
  const uint16_t *ptr = F.P.seg_ptr + (size_t)seg * (ABFT_PANEL_ROWS + 1);
  lo = e0 + ptr[c % ABFT_PANEL_ROWS];
  hi = e0 + ptr[c % ABFT_PANEL_ROWS + 1];
}

// All threads of the calling workgroup (256 or 1024).  Runs behind every COO SpMV -- inside the
// fold of its fused product when there is one, else as coo_fixup_kernel.
__device__ void coo_fixup_body(const FixArgs &fx) {
  __shared__ double s_p[1024];
  __shared__ uint32_t s_o[1024];
  __shared__ uint32_t s_n[1024];
  const CooDev &A = fx.A;
  const uint32_t NT = blockDim.x;
  uint32_t n = __hip_atomic_load(A.moved.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (n == 0u) return;  // uniform
  if (n > A.moved.cap) n = A.moved.cap;
  const MovedEntry *in = A.moved.buf;
  MovedEntry *srt = A.moved.buf + A.moved.cap;
  // rank sort by (column, caller's index); keys are distinct
  for (uint32_t i = threadIdx.x; i < n; i += NT) {
    const MovedEntry e = in[i];
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n; k++) {
      const MovedEntry o = in[k];
      rank += (o.col < e.col || (o.col == e.col && o.orig < e.orig)) ? 1u : 0u;
    }
    srt[rank] = e;
  }
  __threadfence();
  __syncthreads();
  uint32_t q = 0;  // uniform cursor over the sorted entries
  while (q < n) {
    const uint32_t c = srt[q].col;
    uint32_t q1 = q;
    while (q1 < n && srt[q1].col == c) q1++;
    double sum = 0.0;   // thread 0 only
    uint32_t qi = q;    // thread 0 only
    const uint32_t nranges = fx.F.kind == 0 ? 1u : fx.F.P.npanels;
    for (uint32_t rg = 0; rg < nranges; rg++) {
      uint32_t lo, hi;
      fixup_range(A, fx.F, c, rg, lo, hi);
      for (uint32_t base = lo; base < hi; base += NT) {
        const uint32_t j = base + threadIdx.x;
        if (j < hi) {
          const uint4 e = A.elems[j];
          const uint32_t col = fx.ecc ? (e.x & ABFT_COLMASK) : e.x;
          const bool in_range = e.y < A.n_in;
          const double xv = in_range ? fx.x[e.y] : 0.0;
          s_p[threadIdx.x] = as_double(e.z, e.w) * xv;
          s_o[threadIdx.x] = A.orig_index[j];
          s_n[threadIdx.x] = col == c ? 1u : 0u;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
          const uint32_t cnt = min(NT, hi - base);
          for (uint32_t k = 0; k < cnt; k++) {
            if (!s_n[k]) continue;  // moved out itself
            while (qi < q1 && srt[qi].orig < s_o[k]) sum += srt[qi++].prod;
            sum += s_p[k];
          }
        }
        __syncthreads();
      }
    }
    if (threadIdx.x == 0) {
      while (qi < q1) sum += srt[qi++].prod;
      const double old = fx.y[c];
      fx.y[c] = sum;
      if (fx.partial0) {
        const double xo = fx.x[fx.x_off + c];
        *fx.partial0 += xo * sum - xo * old;
      }
    }
    q = q1;
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(A.moved.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(ABFT_BLOCK) void coo_fixup_kernel(FixArgs fx) { coo_fixup_body(fx); }

FixArgs make_fix_args(int mode, const CooDev &A, const CsrPanels *P, const double *x, double *y, const FuseOut *fuse) {
  FixArgs fx{};
  fx.A = A;
  fx.F.kind = P ? 1 : 0;
  if (P) fx.F.P = *P;
  fx.x = x; fx.y = y;
  fx.partial0 = fuse ? fuse->partials : nullptr;
  fx.x_off = fuse ? fuse->x_off : 0u;
  fx.ecc = mode >= MODE_SED;
  fx.on = A.moved.buf && A.nnz ? 1 : 0;
  return fx;
}

hipError_t launch_coo_fixup(const FixArgs &fx, hipStream_t s) {
  if (!fx.on) return hipSuccess;
  hipLaunchKernelGGL(coo_fixup_kernel, dim3(1), dim3(ABFT_BLOCK), 0, s, fx);
  return hipGetLastError();
}

// ------------------------------------------------------------ fault injection --

// The XOR half of inject_bitflip (reference CSR/CPUContext.cpp:146-158); the
// rand() draws stay on the host.
__global__ void inject_csr_kernel(double *vals, uint32_t *cols, const uint32_t *pos_of_orig, uint32_t index,
                                  const int *bits, int nbits) {
  if (blockIdx.x || threadIdx.x) return;
  if (pos_of_orig) index = pos_of_orig[index];  // panel layout: caller's index -> storage position
  uint32_t *vw = reinterpret_cast<uint32_t *>(vals + index);
  for (int k = 0; k < nbits; k++) {
    const int bit = bits[k];
    if (bit < 64) vw[bit >> 5] ^= 1u << (bit & 31);
    else cols[index] ^= 1u << (bit & 31);
  }
}

// reference COO/CPUContext.cpp:134-139
__global__ void inject_coo_kernel(uint4 *elems, const uint32_t *pos_of_orig, uint32_t index,
                                  const int *bits, int nbits) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t *w = reinterpret_cast<uint32_t *>(elems + pos_of_orig[index]);
  for (int k = 0; k < nbits; k++) w[bits[k] >> 5] ^= 1u << (bits[k] & 31);
}

hipError_t launch_inject_csr(double *vals, uint32_t *cols, const uint32_t *pos_of_orig, uint32_t index,
                             const int *bits_dev, int nbits, hipStream_t s) {
  hipLaunchKernelGGL(inject_csr_kernel, dim3(1), dim3(64), 0, s, vals, cols, pos_of_orig, index, bits_dev, nbits);
  return hipGetLastError();
}
hipError_t launch_inject_coo(uint4 *elems, const uint32_t *pos_of_orig, uint32_t index,
                             const int *bits_dev, int nbits, hipStream_t s) {
  hipLaunchKernelGGL(inject_coo_kernel, dim3(1), dim3(64), 0, s, elems, pos_of_orig, index, bits_dev, nbits);
  return hipGetLastError();
}

// ------------------------------------------------------------- vector kernels --

// VEC by alignment: KERNEL<2 MORE> when every operand that enters the test VEC2 is 16-byte aligned, else KERNEL<1 MORE>
// (MORE: the kernel's template arguments after VEC, in parentheses: `()` for none, `(, true)`).  Which operands enter
// the test is each launcher's own matter -- the order a sum is formed in follows the walk.  s: the launcher's stream.
#define ABFT_UNPAREN(...) __VA_ARGS__
#define ABFT_VEC_DISPATCH(KERNEL, MORE, VEC2, NB, ...)                                                               \
  do {                                                                                                               \
    if (VEC2)                                                                                                        \
      hipLaunchKernelGGL((KERNEL<2 ABFT_UNPAREN MORE>), dim3(NB), dim3(ABFT_BLOCK), 0, s, __VA_ARGS__);              \
    else                                                                                                             \
      hipLaunchKernelGGL((KERNEL<1 ABFT_UNPAREN MORE>), dim3(NB), dim3(ABFT_BLOCK), 0, s, __VA_ARGS__);              \
  } while (0)

int reduce_blocks(int n) {
  long per_block = (long)ABFT_BLOCK * 8;  // >= 8 elements per thread before adding blocks
  long nb = (n + per_block - 1) / per_block;
  if (nb < 1) nb = 1;
  if (nb > ABFT_MAX_PARTIALS) nb = ABFT_MAX_PARTIALS;
  return (int)nb;
}

// Second half of every reduction, run by all blocks after their block_sum:
// publish the partial, take a ticket, and let the last arriver combine.
// Inter-workgroup hand-off per the CDNA4 rules, in the cheap form: the partial
// goes out with a write-through (sc1) store -- an agent-scope RELEASE fence here
// would write back every dirty L2 line of the XCD in every block (measured: dot
// 27 -> 81 us, calc_xr 76 -> 175 us) -- the storing lane drains it
// (s_waitcnt vmcnt(0)) before its relaxed agent-scope ticket add; only the last
// arriver pays one agent-scope acquire, drained before the workgroup barrier
// that lets the other lanes read the partials (with sc1 loads).
// The arrival itself (thread 0, its partials already drained): 1 for the block that arrives last.
__device__ __forceinline__ uint32_t reduce_take_ticket(uint32_t *ticket) {
  // two-level arrival: atomics on one address retire one per ~12 ns, so 2048
  // blocks on a single counter cost ~25 us; 32 per group counter (the groups run
  // in parallel) and one top-level add per group cost ~1 us
  const uint32_t g = blockIdx.x / ABFT_TICKET_GROUP, ngroups = (gridDim.x + ABFT_TICKET_GROUP - 1u) / ABFT_TICKET_GROUP;
  const uint32_t gsize = min((uint32_t)ABFT_TICKET_GROUP, gridDim.x - g * ABFT_TICKET_GROUP);
  uint32_t last = 0u;
  if (__hip_atomic_fetch_add(ticket + 1u + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1u) {
    __hip_atomic_store(ticket + 1u + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1u ? 1u : 0u;
  }
  if (last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  return last;
}

// The fold of nb block partials by one whole block, in a fixed order: thread t adds partials t, t + 256, ... ascending,
// then block_sum.  ONE body for the last arriver of reduce_finish and for the blocks of a consumer kernel that finish a
// deferred reduction at their head (deferred_head): the same partials give the same bits wherever they are folded.
// (AGENT: loads that pass the L1, for partials other blocks of this launch stored; a deferred reduction's partials
// were stored by an earlier launch and are read plainly, so that the blocks of one CU share them in its L1)
template <bool AGENT>
__device__ __forceinline__ double fold_block_partials(const double *partials, uint32_t nb, double *s_w) {
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < nb; i += ABFT_BLOCK)  // fixed order
    acc += AGENT ? __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : partials[i];
  return block_sum(acc, s_w);
}

// {value, queued events} into the pinned slot (one thread): write-through system-scope stores, drained, then the
// sequence number: the host sees {value, evcount} before seq without a release fence (which would first write back
// every dirty line calc_xr left in this XCD's L2)
__device__ __forceinline__ void publish_host(HostSlot *host, double value, uint32_t nev, uint32_t seq) {
  __hip_atomic_store(&host->value, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host->evcount, nev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&host->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void reduce_finish(double block_value, const ReduceOut &o, double *s_w) {
  __shared__ uint32_t s_last;
  if (threadIdx.x == 0) {
    __hip_atomic_store(o.partials + blockIdx.x, block_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = reduce_take_ticket(o.ticket);
  }
  __syncthreads();
  if (!s_last) return;
  double acc = fold_block_partials<true>(o.partials, gridDim.x, s_w);
  uint32_t nev = 0u;
  double evs = 0.0;
  if (threadIdx.x == 0) {
    nev = __hip_atomic_load(o.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    evs = (double)nev;
  }
  if (o.peers.size) peer_allreduce_block(acc, evs, o.peers);  // the whole (last) block; uniform: a kernel argument
  if (threadIdx.x == 0) {
    if (o.dev_out) {  // {sum, queued events} of this shard -- or of all ranks, when the board is in the tail
      o.dev_out[0] = acc;
      o.dev_out[1] = evs;
    }
    __hip_atomic_store(o.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    if (o.host) publish_host(o.host, acc, nev, o.seq);
  }
}

// ---- a reduction finished by the kernel behind it ----
// When the kernel that consumes a reduction's result is enqueued in the same call, the producer needs no last
// arriver: its blocks leave their partials with plain stores and end (no drain, no ticket), and EVERY block of the
// consumer folds them at its head, by fold_block_partials as the last arriver would have -- the same bits in every
// block.  Block 0 of the consumer publishes what reduce_finish publishes: {sum, queued events} to o.dev_out and to the
// pinned slot.  The kernel boundary is the hand-off: o.partials belongs to this reduction until the consumer has ended
// (abft_hip.hip keeps one area per deferred reduction).  No peers: the single-process loop only.
// (o: the producer's ReduceOut; ticket unused.  s_h: four doubles of LDS that nothing else in the kernel uses)
__device__ __forceinline__ double deferred_head(const ReduceOut &o, uint32_t nb, double *s_h) {
  const double acc = fold_block_partials<false>(o.partials, nb, s_h);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t nev = __hip_atomic_load(o.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o.dev_out) {
      o.dev_out[0] = acc;
      o.dev_out[1] = (double)nev;
    }
    if (o.host) publish_host(o.host, acc, nev, o.seq);
  }
  return acc;
}

// the head alone, in one block: behind a deferred producer whose consumer could not be launched, so that the host
// never waits on a slot nobody writes
__global__ __launch_bounds__(ABFT_BLOCK) void deferred_finish_kernel(ReduceOut o, uint32_t nb) {
  __shared__ double s_h[4];
  (void)deferred_head(o, nb, s_h);
}

hipError_t launch_deferred_finish(const ReduceOut &o, uint32_t nb, hipStream_t s) {
  hipLaunchKernelGGL(deferred_finish_kernel, dim3(1), dim3(ABFT_BLOCK), 0, s, o, nb);
  return hipGetLastError();
}

// Fold of many fused-dot partials (config 2: 48 806 of them, 390 KB) by several
// workgroups: one workgroup reads at one CU's bandwidth and took 8-10 us.  Each
// workgroup adds a contiguous chunk in a fixed order, then the chunks' sums meet
// through the same last-arriver protocol as every other reduction.

// One column's sum over this workgroup's chunk [lo, hi) of the partials at pj, in a fixed order.  The one body of
// fold_partials_kernel, spmm_fold_kernel and spmm_fold_dev_kernel.
__device__ __forceinline__ double fold_chunk_sum(const double *__restrict__ pj, uint32_t lo, uint32_t hi) {
  double a = 0.0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 4u * ABFT_BLOCK) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t q = i + (uint32_t)u * ABFT_BLOCK;
      v[u] = q < hi ? pj[q] : 0.0;
    }
    a += (v[0] + v[1]) + (v[2] + v[3]);
  }
  return a;
}

// The grid of a multi-workgroup fold of nblk partials: one workgroup per 2048 partials, 64 at most, each with a
// contiguous chunk.  The one rule of fold_partials_kernel, spmm_fold_kernel, spmm_fold_dev_kernel and the fold that
// abft_hip_cg_iteration_dev releases after its SpMV.
uint32_t fold_grid(uint32_t nblk, uint32_t *chunk) {
  uint32_t nb = (nblk + 2047u) / 2048u;
  if (nb < 1u) nb = 1u;
  if (nb > 64u) nb = 64u;
  *chunk = (nblk + nb - 1u) / nb;
  return nb;
}

__global__ __launch_bounds__(ABFT_BLOCK) void fold_partials_kernel(const double *__restrict__ parts, uint32_t n,
                                                                   uint32_t chunk, ReduceOut out, FixArgs fx) {
  __shared__ double s_w[4];
  if (fx.on && blockIdx.x == 0) coo_fixup_body(fx);  // workgroup 0 owns partial 0, which the fix-up corrects
  const uint32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  double acc = fold_chunk_sum(parts, lo, hi);
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// fold_partials_kernel with its finish left to the kernel behind it (deferred_head): the chunk sums, and no more
__global__ __launch_bounds__(ABFT_BLOCK) void fold_partials_defer_kernel(const double *__restrict__ parts, uint32_t n,
                                                                         uint32_t chunk, double *chunk_sums,
                                                                         FixArgs fx) {
  __shared__ double s_w[4];
  if (fx.on && blockIdx.x == 0) coo_fixup_body(fx);
  const uint32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  double acc = fold_chunk_sum(parts, lo, hi);
  acc = block_sum(acc, s_w);
  if (threadIdx.x == 0) chunk_sums[blockIdx.x] = acc;
}

bool fuse_finalize_folds(uint32_t nblk) { return nblk > 8192u; }

hipError_t launch_fuse_finalize(const FuseOut &f, uint32_t nblk, const ReduceOut &big, const FixArgs *fix,
                                hipStream_t s) {
  FixArgs fx{};
  if (fix) fx = *fix;
  if (!fuse_finalize_folds(nblk) || !big.partials) {
    hipLaunchKernelGGL(fuse_finalize_kernel, dim3(1), dim3(1024), 0, s, f, nblk, fx);
    return hipGetLastError();
  }
  uint32_t chunk;
  const uint32_t nb = fold_grid(nblk, &chunk);
#ifdef ABFT_DBG_DEFER_ALWAYS  // timing build: every multi-workgroup fold without its tail, a one-block finisher behind it
  hipLaunchKernelGGL(fold_partials_defer_kernel, dim3(nb), dim3(ABFT_BLOCK), 0, s, f.partials, nblk, chunk, big.partials, fx);
  return launch_deferred_finish(big, nb, s);
#endif
  hipLaunchKernelGGL(fold_partials_kernel, dim3(nb), dim3(ABFT_BLOCK), 0, s, f.partials, nblk, chunk, big, fx);
  return hipGetLastError();
}

hipError_t launch_fuse_finalize_defer(const FuseOut &f, uint32_t nblk, double *chunk_sums, const FixArgs *fix,
                                      uint32_t *nb_out, hipStream_t s) {
  FixArgs fx{};
  if (fix) fx = *fix;
  uint32_t chunk;
  const uint32_t nb = fold_grid(nblk, &chunk);
  *nb_out = nb;
  hipLaunchKernelGGL(fold_partials_defer_kernel, dim3(nb), dim3(ABFT_BLOCK), 0, s, f.partials, nblk, chunk, chunk_sums, fx);
  return hipGetLastError();
}

// dot (reference CSR/CPUContext.cpp:82-90).  VEC=2: 16-byte loads.
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void dot_kernel(const double *__restrict__ a,
                                                         const double *__restrict__ b, int n,
                                                         ReduceOut out) {
  __shared__ double s_w[4];
  double acc = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      const double2 av = *reinterpret_cast<const double2 *>(a + i);
      const double2 bv = *reinterpret_cast<const double2 *>(b + i);
      acc += av.x * bv.x;
      acc += av.y * bv.y;
    } else {
      acc += a[i] * b[i];
    }
  }
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// calc_xr (reference CSR/CPUContext.cpp:92-105): x += alpha p; r -= alpha w;
// r.r with the updated r.
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_xr_kernel(double *__restrict__ x, double *__restrict__ r,
                                                             const double *__restrict__ p,
                                                             const double *__restrict__ w, double alpha,
                                                             const double *num, const double *den, int n,
                                                             ReduceOut out) {
  __shared__ double s_w[4];
  if (num) alpha = *num / *den;  // alpha = rr / pw formed on the device (cg.cpp:102)
  double acc = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 xv = *reinterpret_cast<double2 *>(x + i);
      double2 rv = *reinterpret_cast<double2 *>(r + i);
      const double2 pv = *reinterpret_cast<const double2 *>(p + i);
      const double2 wv = *reinterpret_cast<const double2 *>(w + i);
      xv.x += alpha * pv.x; xv.y += alpha * pv.y;
      rv.x -= alpha * wv.x; rv.y -= alpha * wv.y;
      *reinterpret_cast<double2 *>(x + i) = xv;
      *reinterpret_cast<double2 *>(r + i) = rv;
      acc += rv.x * rv.x;
      acc += rv.y * rv.y;
    } else {
      const double xs = x[i] + alpha * p[i];
      const double rs = r[i] - alpha * w[i];
      x[i] = xs;
      r[i] = rs;
      acc += rs * rs;
    }
  }
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// calc_p (reference CSR/CPUContext.cpp:107-113): p = r + beta p
// (p_out: where the new p goes -- p itself, or the buffer p's handle is about to swap to while the old p waits
// for the SpMV that applies x += alpha p_old, abft_hip.hip "xpend")
// The walk of calc_p_kernel and calc_p_head_kernel: p_out = r + beta p over the grid.
// (PRE: this thread's first pair of p and r was loaded by the caller -- before it knew beta -- into p0, r0)
template <int VEC, bool PRE>
__device__ __forceinline__ void calc_p_walk(const double *p, const double *__restrict__ r, double beta, int n,
                                            double *p_out, double2 p0, double2 r0) {
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  const long start = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC;
  for (long i = start; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      const bool pre = PRE && i == start;
      double2 pv = pre ? p0 : *reinterpret_cast<const double2 *>(p + i);
      const double2 rv = pre ? r0 : *reinterpret_cast<const double2 *>(r + i);
      pv.x = rv.x + beta * pv.x;
      pv.y = rv.y + beta * pv.y;
#if ABFT_CFG_P_OUT_NT
      typedef double v2d __attribute__((ext_vector_type(2)));
      if (p_out != p) __builtin_nontemporal_store(v2d{pv.x, pv.y}, reinterpret_cast<v2d *>(p_out + i));
      else *reinterpret_cast<double2 *>(p_out + i) = pv;
#else
      *reinterpret_cast<double2 *>(p_out + i) = pv;
#endif
    } else {
      p_out[i] = r[i] + beta * p[i];
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_p_kernel(const double *p, const double *__restrict__ r,
                                                            double beta, const double *num, const double *den,
                                                            int n, double *p_out) {
  if (num) beta = *num / *den;  // beta = rr_new / rr formed on the device (cg.cpp:109)
  calc_p_walk<VEC, false>(p, r, beta, n, p_out, double2{}, double2{});
}

// calc_p behind a calc_r that left its r.r to this kernel (deferred_head): every block folds the nb block partials
// behind its first loads of p and r, beta = r.r_new / *den -- the division calc_p_kernel does with *num --, block 0
// publishes {r.r_new, queued events}; then calc_p_kernel's walk.
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_p_head_kernel(const double *p, const double *__restrict__ r,
                                                                 const double *den, int n, double *p_out,
                                                                 ReduceOut head, uint32_t nb) {
  __shared__ double s_h[4];
  const long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC;
  double2 pv = make_double2(0.0, 0.0), rv = pv;
  if (VEC == 2 && i + 1 < n) {
    pv = *reinterpret_cast<const double2 *>(p + i);
    rv = *reinterpret_cast<const double2 *>(r + i);
  }
  const double rr = *den;
  const double beta = deferred_head(head, nb, s_h) / rr;
  calc_p_walk<VEC, true>(p, r, beta, n, p_out, pv, rv);
}

static inline bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr,
                             const void *d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15u) == 0;
}

hipError_t launch_dot(const double *a, const double *b, int n, const ReduceOut &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(dot_kernel, (), aligned16(a, b), nb, a, b, n, out);
  return hipGetLastError();
}

hipError_t launch_calc_xr(double *x, double *r, const double *p, const double *w, double alpha,
                          const double *num, const double *den, int n, const ReduceOut &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_xr_kernel, (), aligned16(x, r, p, w), nb, x, r, p, w, alpha, num, den, n, out);
  return hipGetLastError();
}

hipError_t launch_calc_p(double *p, const double *r, double beta, const double *num, const double *den, int n,
                         hipStream_t s, double *p_out) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  if (!p_out) p_out = p;
  ABFT_VEC_DISPATCH(calc_p_kernel, (), aligned16(p, r, p_out), nb, p, r, beta, num, den, n, p_out);
  return hipGetLastError();
}

// (head, nb: the ReduceOut and the grid of the calc_r whose r.r this launch finishes, launch_calc_r_defer)
hipError_t launch_calc_p_head(const double *p, const double *r, const double *den, int n, hipStream_t s, double *p_out,
                              const ReduceOut &head, uint32_t nb) {
  const int g = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_p_head_kernel, (), aligned16(p, r, p_out), g, p, r, den, n, p_out, head, nb);
  return hipGetLastError();
}

// ---- calc_xr / calc_p with the x update moved (cross-call fusion, abft_hip.hip) ----
// calc_xr reads p only for x += alpha p, and the calc_p that follows it in the CG loop
// reads the same p again.  When the library sees that pair it runs calc_xr without its
// x half (calc_r_kernel: 24 N bytes instead of 48 N) and lets calc_p do it
// (calc_px_kernel: 40 N instead of 24 N) -- p is read once per iteration, 8 N bytes
// less traffic, every x[i] and p[i] the same bits (same operands, same two roundings).

// The walk of calc_r_kernel and calc_r_until_kernel: r_out = r - alpha w over the grid, -> this thread's serial sum of
// the new r's squares.  ONE body, so that the guarded kernel cannot drift from the one it must match bit for bit.
// (r_out: where the updated r goes -- r itself, or the shadow buffer of a speculated iteration, abft_hip.hip "speculation")
template <int VEC>
__device__ __forceinline__ double calc_r_walk(const double *r, const double *__restrict__ w, double alpha, int n,
                                              double *r_out) {
  double acc = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 rv = *reinterpret_cast<const double2 *>(r + i);
#if ABFT_CFG_DEAD_NT & 1  // w is dead after this read (the next SpMV rewrites it)
      typedef double v2d __attribute__((ext_vector_type(2)));
      const v2d wl = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(w + i));
      const double2 wv = make_double2(wl.x, wl.y);
#else
      const double2 wv = *reinterpret_cast<const double2 *>(w + i);
#endif
      rv.x -= alpha * wv.x; rv.y -= alpha * wv.y;
#if ABFT_CFG_R_NT  // bit 0: the store into the shadow of a run-ahead (r_out != r), bit 1: the store in place
      typedef double v2r __attribute__((ext_vector_type(2)));
      if ((ABFT_CFG_R_NT & 1) && r_out != r) __builtin_nontemporal_store(v2r{rv.x, rv.y}, reinterpret_cast<v2r *>(r_out + i));
      else if ((ABFT_CFG_R_NT & 2) && r_out == r) __builtin_nontemporal_store(v2r{rv.x, rv.y}, reinterpret_cast<v2r *>(r_out + i));
      else *reinterpret_cast<double2 *>(r_out + i) = rv;
#else
      *reinterpret_cast<double2 *>(r_out + i) = rv;
#endif
      acc += rv.x * rv.x;
      acc += rv.y * rv.y;
    } else {
      const double rs = r[i] - alpha * w[i];
      r_out[i] = rs;
      acc += rs * rs;
    }
  }
  return acc;
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_kernel(const double *r, const double *__restrict__ w,
                                                            double alpha, const double *num, const double *den,
                                                            double *alpha_out, int n, ReduceOut out, double *r_out) {
  __shared__ double s_w[4];
  if (num) alpha = *num / *den;
  if (alpha_out && blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = alpha;  // for the deferred x += alpha p
  double acc = calc_r_walk<VEC>(r, w, alpha, n, r_out);
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// calc_r_kernel with its finish left to the kernel behind it (calc_p_head_kernel, or deferred_finish_kernel): the
// same walk and block_sum, the block's partial stored plainly, and the kernel ends.
// HEAD: it also finishes the deferred fold of the fused p.w in front of it (fold_partials_defer_kernel):
// alpha = *num / p.w, the division calc_r_kernel does with *den; block 0 publishes {p.w, queued events}.
template <int VEC, bool HEAD>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_defer_kernel(const double *r, const double *__restrict__ w,
                                                                  double alpha, const double *num, const double *den,
                                                                  double *alpha_out, int n, double *block_partials,
                                                                  double *r_out, ReduceOut head, uint32_t nb) {
  __shared__ double s_w[4];
  if (HEAD) {
    __shared__ double s_h[4];
    const double rr = *num;
    alpha = rr / deferred_head(head, nb, s_h);
  } else if (num) {
    alpha = *num / *den;
  }
  if (alpha_out && blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = alpha;
  double acc = calc_r_walk<VEC>(r, w, alpha, n, r_out);
  acc = block_sum(acc, s_w);
  if (threadIdx.x == 0) block_partials[blockIdx.x] = acc;
}

// The walk of calc_px_kernel and calc_px_until_kernel: x_out = x + alpha p, p_out = r + beta p, p read once.
// (p_out, x_out: where the new p and x go -- p and x themselves, or the shadow buffers of a speculated iteration)
template <int VEC>
__device__ __forceinline__ void calc_px_walk(const double *p, const double *__restrict__ r, const double *x,
                                             double beta, double alpha, int n, double *p_out, double *x_out) {
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
#if ABFT_CFG_X_NT || (ABFT_CFG_DEAD_NT & 6) || ABFT_CFG_PX_OUT_NT
      typedef double v2d __attribute__((ext_vector_type(2)));
#endif
#if ABFT_CFG_DEAD_NT & 4  // the old p is dead after this read
      const v2d pl = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(p + i));
      double2 pv = make_double2(pl.x, pl.y);
#else
      double2 pv = *reinterpret_cast<const double2 *>(p + i);
#endif
#if ABFT_CFG_X_NT  // x is touched once per iteration: keep it out of the caches (Infinity Cache included) that p, r, w could live in
      const v2d xl = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(x + i));
      double2 xv = make_double2(xl.x, xl.y);
#else
      double2 xv = *reinterpret_cast<const double2 *>(x + i);
#endif
#if ABFT_CFG_DEAD_NT & 2  // r is not read again before the next iteration's calc_r rewrites it
      const v2d rl = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(r + i));
      const double2 rv = make_double2(rl.x, rl.y);
#else
      const double2 rv = *reinterpret_cast<const double2 *>(r + i);
#endif
      xv.x += alpha * pv.x; xv.y += alpha * pv.y;  // calc_xr's x half, with p as calc_xr saw it
      pv.x = rv.x + beta * pv.x;
      pv.y = rv.y + beta * pv.y;
#if ABFT_CFG_X_NT
      __builtin_nontemporal_store(v2d{xv.x, xv.y}, reinterpret_cast<v2d *>(x_out + i));
#elif ABFT_CFG_PX_OUT_NT & 1
      if (x_out != x) __builtin_nontemporal_store(v2d{xv.x, xv.y}, reinterpret_cast<v2d *>(x_out + i));
      else *reinterpret_cast<double2 *>(x_out + i) = xv;
#else
      *reinterpret_cast<double2 *>(x_out + i) = xv;
#endif
#if ABFT_CFG_PX_OUT_NT & 2
      if (p_out != p) __builtin_nontemporal_store(v2d{pv.x, pv.y}, reinterpret_cast<v2d *>(p_out + i));
      else *reinterpret_cast<double2 *>(p_out + i) = pv;
#else
      *reinterpret_cast<double2 *>(p_out + i) = pv;
#endif
    } else {
      const double pv = p[i];
      x_out[i] = x[i] + alpha * pv;
      p_out[i] = r[i] + beta * pv;
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_kernel(const double *p, const double *__restrict__ r,
                                                             const double *x, double beta,
                                                             const double *num, const double *den, double alpha,
                                                             const double *alpha_ptr, int n, double *p_out, double *x_out) {
  if (num) beta = *num / *den;
  if (alpha_ptr) alpha = *alpha_ptr;
  calc_px_walk<VEC>(p, r, x, beta, alpha, n, p_out, x_out);
}

// the deferred x += alpha p on its own, when something other than calc_p comes next
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void axpy_kernel(double *__restrict__ x, const double *__restrict__ p,
                                                          double alpha, const double *alpha_ptr, int n) {
  if (alpha_ptr) alpha = *alpha_ptr;
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 xv = *reinterpret_cast<double2 *>(x + i);
      const double2 pv = *reinterpret_cast<const double2 *>(p + i);
      xv.x += alpha * pv.x; xv.y += alpha * pv.y;
      *reinterpret_cast<double2 *>(x + i) = xv;
    } else {
      x[i] = x[i] + alpha * p[i];
    }
  }
}

// the queued updates x += a0 p0; x += a1 p1; ... on their own (loop_state.h, LazyUpdates): axpy_kernel
// u.n times -- per element the same multiplies and adds in the same order -- with x read once and written once
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void axpy_chain_kernel(XUpd u, int n) {
  double *x = u.xs;
  const int cnt = u.n;  // uniform
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 xv = *reinterpret_cast<double2 *>(x + i);
      for (int k = 0; k < cnt; k++) {
        const double2 pv = *reinterpret_cast<const double2 *>(u.u[k].p_old + i);
        xv.x += u.u[k].alpha * pv.x; xv.y += u.u[k].alpha * pv.y;
      }
      *reinterpret_cast<double2 *>(x + i) = xv;
    } else {
      double xv = x[i];
      for (int k = 0; k < cnt; k++) xv = xv + u.u[k].alpha * u.u[k].p_old[i];
      x[i] = xv;
    }
  }
}

// (x, p: the operands of the calc_xr this is the r half of.  The kernel does not touch them, but the order in which r.r
// is summed follows the walk, and the walk is chosen over all four operands -- as calc_xr_kernel's and cg_tail_kernel's
// is -- so that the sum has the same bits whichever of the three runs the call)
hipError_t launch_calc_r(double *r, const double *w, double alpha, const double *num, const double *den,
                         double *alpha_out, int n, const ReduceOut &out, hipStream_t s, double *r_out, const double *x,
                         const double *p) {
  const int nb = reduce_blocks(n);
  if (!r_out) r_out = r;
#ifdef ABFT_DBG_DEFER_ALWAYS  // timing build: every calc_r without its tail, a one-block finisher behind it
  if (!out.peers.size) {
    if (hipError_t e = launch_calc_r_defer(r, w, alpha, num, den, alpha_out, n, out.partials, s, r_out, x, p, nullptr, 0u))
      return e;
    return launch_deferred_finish(out, (uint32_t)nb, s);
  }
#endif
  ABFT_VEC_DISPATCH(calc_r_kernel, (), aligned16(r, w, r_out) && aligned16(x, p), nb, r, w, alpha, num, den, alpha_out,
                    n, out, r_out);
  return hipGetLastError();
}

// launch_calc_r with the finish of r.r left to the launch behind it: the block partials go to block_partials
// (reduce_blocks(n) of them), which launch_calc_p_head or launch_deferred_finish folds.
// head != nullptr: it finishes the deferred fold in front of it (launch_fuse_finalize_defer: head_nb chunk sums at
// head->partials) and divides *num by that p.w; den is not read.
hipError_t launch_calc_r_defer(double *r, const double *w, double alpha, const double *num, const double *den,
                               double *alpha_out, int n, double *block_partials, hipStream_t s, double *r_out,
                               const double *x, const double *p, const ReduceOut *head, uint32_t head_nb) {
  const int nb = reduce_blocks(n);
  if (!r_out) r_out = r;
  const bool vec2 = aligned16(r, w, r_out) && aligned16(x, p);
  if (head) {
    ABFT_VEC_DISPATCH(calc_r_defer_kernel, (, true), vec2, nb, r, w, alpha, num, den, alpha_out, n, block_partials, r_out,
                      *head, head_nb);
  } else {
    const ReduceOut none{};
    ABFT_VEC_DISPATCH(calc_r_defer_kernel, (, false), vec2, nb, r, w, alpha, num, den, alpha_out, n, block_partials, r_out,
                      none, 0u);
  }
  return hipGetLastError();
}

hipError_t launch_calc_px(double *p, const double *r, double *x, double beta, const double *num, const double *den,
                          double alpha, const double *alpha_ptr, int n, hipStream_t s, double *p_out, double *x_out) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  if (!p_out) p_out = p;
  if (!x_out) x_out = x;
  ABFT_VEC_DISPATCH(calc_px_kernel, (), aligned16(p, r, x) && aligned16(p_out, x_out), nb, p, r, x, beta, num, den,
                    alpha, alpha_ptr, n, p_out, x_out);
  return hipGetLastError();
}

hipError_t launch_axpy(double *x, const double *p, double alpha, const double *alpha_ptr, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(axpy_kernel, (), aligned16(x, p), nb, x, p, alpha, alpha_ptr, n);
  return hipGetLastError();
}

hipError_t launch_axpy_chain(const XUpd &u, int n, hipStream_t s) {
  if (u.n < 1 || u.n > 4 || !u.xs) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  bool vec2 = aligned16(u.xs);
  for (int k = 0; k < u.n; k++) {
    if (!u.u[k].p_old) return hipErrorInvalidValue;
    vec2 = vec2 && aligned16(u.u[k].p_old);
  }
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(axpy_chain_kernel, (), vec2, nb, u, n);
  return hipGetLastError();
}

// ---- the guarded iteration (abft_hip_cg_iteration_until_dev) ----
// calc_r_kernel and calc_px_kernel behind the stop test that guard_protocol.h states, on GuardPair records.  A live
// launch walks, computes and reduces exactly as the unguarded kernel does on the same grid: same bits everywhere.
// (Kernels with symbols of their own and not a template flag on the two above; the streaming loop is the one body
// calc_r_walk / calc_px_walk, called with r_out = r, p_out = p, x_out = x.)

// The head of every single r half (REC: GuardPair, GuardQuad; Out: ReduceOut, ReduceOutD): frozen -> false, the record
// handed on by one thread; live -> true with alpha, which one thread leaves in *alpha_out for the x / p half.
template <class REC, class Out>
__device__ __forceinline__ bool guard_r_head(const double *in, const double *pw, double threshold, double *alpha_out,
                                             const Out &out, double *alpha) {
  if (!REC::live(in, threshold)) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      REC::hand_on(in, out.dev_out, __hip_atomic_load(out.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return false;
  }
  *alpha = REC::alpha(in, *pw);
  if (blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = *alpha;
  return true;
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_until_kernel(double *r, const double *__restrict__ w,
                                                                  const double *rr, const double *pw,
                                                                  double threshold, double *alpha_out, int n,
                                                                  ReduceOut out) {
  __shared__ double s_w[4];
  double alpha;
  if (!guard_r_head<GuardPair>(rr, pw, threshold, alpha_out, out, &alpha)) return;
  double acc = calc_r_walk<VEC>(r, w, alpha, n, r);
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_until_kernel(double *p, const double *__restrict__ r, double *x,
                                                                   const double *rr, const double *rr_new,
                                                                   double threshold, const double *alpha_ptr, int n) {
  if (!GuardPair::live(rr, threshold)) return;
  const double beta = GuardPair::beta(rr, rr_new);
  const double alpha = *alpha_ptr;
  calc_px_walk<VEC>(p, r, x, beta, alpha, n, p, x);
}

// (the walk is chosen over all four operands in both launches, as launch_calc_r's is: r.r is summed in the same order)
hipError_t launch_calc_r_until(double *r, const double *w, const double *rr, const double *pw, double threshold,
                               double *alpha_out, int n, const ReduceOut &out, hipStream_t s, const double *x,
                               const double *p) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_r_until_kernel, (), aligned16(r, w, x, p), nb, r, w, rr, pw, threshold, alpha_out, n, out);
  return hipGetLastError();
}

hipError_t launch_calc_px_until(double *p, const double *r, double *x, const double *rr, const double *rr_new,
                                double threshold, const double *alpha_ptr, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_px_until_kernel, (), aligned16(p, r, x), nb, p, r, x, rr, rr_new, threshold, alpha_ptr, n);
  return hipGetLastError();
}

// ---- block vectors (K right-hand sides, row-major: entry (i, j) at i*K + j) ----
// One thread per row i walks rows exactly as the single kernels' threads walk elements (grid
// reduce_blocks(n rows)); per column the same operations with the same roundings, so an active
// column's elements are the bits calc_xr_kernel / calc_p_kernel give for it.  A column whose bit
// is clear in `active` is written back with the bits it was read with (a select, never an
// arithmetic operation: inf and NaN payloads survive).  The K reductions have ONE shape: per
// thread a serial sum over its rows, block_sum, then the last-arriving block's fixed-order fold
// of the block partials -- so scaling a column by a power of two scales its sum by the same
// power exactly.  Results: K doubles + the queued-event count in a K-wide pinned slot.
template <int K>
__device__ __forceinline__ void block_load(const double *p, double *v) {
  if (K % 2 == 0) {
#pragma unroll
    for (int j = 0; j < K; j += 2) {
      const double2 t = *reinterpret_cast<const double2 *>(p + j);
      v[j] = t.x; v[j + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; j++) v[j] = p[j];
  }
}

template <int K>
__device__ __forceinline__ void block_store(double *p, const double *v) {
  if (K % 2 == 0) {
#pragma unroll
    for (int j = 0; j < K; j += 2) *reinterpret_cast<double2 *>(p + j) = make_double2(v[j], v[j + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < K; j++) p[j] = v[j];
  }
}

// reduce_finish for K values: K partials per block, one ticket, K fixed-order folds.  The ONE routine every K-wide
// reduction goes through: block sums, partial stores, the drained ticket, the last-arriving block's fixed-order folds.
// -> true in the last-arriving block with the K totals (valid in every thread's copy, as block_sum leaves them),
// false elsewhere.  Thread 0 of that block then publishes: reduce_rearm, and one of the publishers below, which
// differ only in where the totals go.  (Out: ReduceOutK, ReduceOutW, ReduceOutD or ReduceOutB)
// (Last: the type the answer comes back in, bool or uint32_t -- the same answer.  It is here for the register
// allocator alone: with uint32_t the kernels that publish a ReduceOutB record get the branch on s_last as a scalar
// one and 2-6 fewer VGPRs, as they had with a routine of their own; with bool every pinned-slot kernel keeps the
// instructions it had.  DESIGN 5i has the table.)
template <int K, class Out, class Last = bool>
__device__ __forceinline__ Last reduce_totals_k(const double *value, const Out &o, double *s_w, double *tot) {
  __shared__ uint32_t s_last;
  double bv[K];
#pragma unroll
  for (int j = 0; j < K; j++) bv[j] = block_sum(value[j], s_w + 4 * j);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < K; j++)
      __hip_atomic_store(o.partials + (size_t)j * ABFT_MAX_PARTIALS + blockIdx.x, bv[j], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = reduce_take_ticket(o.ticket);
  }
  __syncthreads();
  if (!s_last) return Last(0);
#pragma unroll
  for (int j = 0; j < K; j++) {
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += ABFT_BLOCK)  // fixed order
      acc += __hip_atomic_load(o.partials + (size_t)j * ABFT_MAX_PARTIALS + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tot[j] = block_sum(acc, s_w + 4 * (K + j));
  }
  return Last(1);
}

// the publishing thread's first two steps: -> the queued-event count, the ticket ready for the next launch
template <class Out>
__device__ __forceinline__ uint32_t reduce_rearm(const Out &o) {
  const uint32_t nev = __hip_atomic_load(o.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(o.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return nev;
}

// publisher: the K totals and the event count into the K-wide pinned slot
// (Out: ReduceOutK, or ReduceOutW for the 2K sums of a block residual check)
template <int K, class Out = ReduceOutK>
__device__ __forceinline__ void reduce_finish_k(const double *value, const Out &o, double *s_w) {
  double tot[K];
  if (!reduce_totals_k<K>(value, o, s_w, tot) || threadIdx.x != 0) return;
  const uint32_t nev = reduce_rearm(o);
#pragma unroll
  for (int j = 0; j < K; j++)
    __hip_atomic_store(&o.host->value[j], tot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&o.host->evcount, nev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&o.host->seq, o.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// publisher: two totals, value[0] = r.z and value[1] = r.r, into the device record of four doubles
__device__ __forceinline__ void reduce_finish_d(const double *value, const ReduceOutD &o, double *s_w) {
  double tot[2];
  if (!reduce_totals_k<2>(value, o, s_w, tot) || threadIdx.x != 0) return;
  const uint32_t nev = reduce_rearm(o);
  o.dev_out[0] = tot[1];
  o.dev_out[1] = (double)nev;
  o.dev_out[2] = tot[0];
  o.dev_out[3] = 0.0;
}

// publisher: the K totals and the event count into the block record {K totals, queued events}
template <int K>
__device__ __forceinline__ void reduce_finish_b(const double *value, const ReduceOutB &o, double *s_w) {
  double tot[K];
  if (!reduce_totals_k<K, ReduceOutB, uint32_t>(value, o, s_w, tot)) return;
  if (threadIdx.x == 0) {
    const uint32_t nev = reduce_rearm(o);
#pragma unroll
    for (int j = 0; j < K; j++) o.dev_out[j] = tot[j];
    o.dev_out[K] = (double)nev;
  }
}

template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void dot_block_kernel(const double *__restrict__ a,
                                                               const double *__restrict__ b, int n, ReduceOutK out) {
  __shared__ double s_w[8 * K];
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double av[K], bv[K];
    block_load<K>(a + i * K, av);
    block_load<K>(b + i * K, bv);
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] += av[j] * bv[j];
  }
  reduce_finish_k<K>(acc, out, s_w);
}

template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_xr_block_kernel(double *__restrict__ x, double *__restrict__ r,
                                                                   const double *__restrict__ p,
                                                                   const double *__restrict__ w, BlockScalars alpha,
                                                                   uint32_t active, int n, ReduceOutK out) {
  __shared__ double s_w[8 * K];
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double xv[K], rv[K], pv[K], wv[K];
    block_load<K>(x + i * K, xv);
    block_load<K>(r + i * K, rv);
    block_load<K>(p + i * K, pv);
    block_load<K>(w + i * K, wv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const bool on = (active >> j) & 1u;
      const double xs = xv[j] + alpha.v[j] * pv[j];  // calc_xr_kernel's two roundings
      const double rs = rv[j] - alpha.v[j] * wv[j];
      xv[j] = on ? xs : xv[j];
      rv[j] = on ? rs : rv[j];
      acc[j] += rv[j] * rv[j];
    }
    block_store<K>(x + i * K, xv);
    block_store<K>(r + i * K, rv);
  }
  reduce_finish_k<K>(acc, out, s_w);
}

template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_p_block_kernel(double *__restrict__ p, const double *__restrict__ r,
                                                                  BlockScalars beta, uint32_t active, int n) {
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double pv[K], rv[K];
    block_load<K>(p + i * K, pv);
    block_load<K>(r + i * K, rv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const double ps = rv[j] + beta.v[j] * pv[j];
      pv[j] = ((active >> j) & 1u) ? ps : pv[j];
    }
    block_store<K>(p + i * K, pv);
  }
}

#define ABFT_BLOCK_K_DISPATCH(OP) \
  switch (k) {                    \
    case 1: OP(1); break;         \
    case 2: OP(2); break;         \
    case 3: OP(3); break;         \
    case 4: OP(4); break;         \
    case 5: OP(5); break;         \
    case 6: OP(6); break;         \
    case 7: OP(7); break;         \
    case 8: OP(8); break;         \
    default: return hipErrorInvalidValue; \
  }

hipError_t launch_dot_block(const double *a, const double *b, int n, int k, const ReduceOutK &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) hipLaunchKernelGGL(dot_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, a, b, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_xr_block(double *x, double *r, const double *p, const double *w, int n, int k,
                                const BlockScalars &alpha, uint32_t active, const ReduceOutK &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL(calc_xr_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, x, r, p, w, alpha, active, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_p_block(double *p, const double *r, int n, int k, const BlockScalars &beta, uint32_t active,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) hipLaunchKernelGGL(calc_p_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, p, r, beta, active, n)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// ---- residual checks: the recurrence's r against the true residual b - A x ----
// The SpMV half of a check is the ordinary one (y = A x into the dead w); these kernels are the
// one pass behind it.  Single vectors walk elements exactly as dot_kernel<VEC> does, block vectors
// walk rows exactly as dot_block_kernel<K> does, with the same reductions.

// XOR `mask` into one double (fault injection into a vector: tests and the CLI's --flip-vector)
__global__ void flip_vector_kernel(double *v, unsigned long long mask) {
  *v = __longlong_as_double(__double_as_longlong(*v) ^ (long long)mask);
}

// {gap2, tt2} = {sum ((b - y) - r)^2, sum (b - y)^2}.  (b - y) - r in that order: with r equal to the
// rounded b - y the gap of every element is exactly 0.
// (the element walk, shared by residual_gap_kernel and residual_check_kernel as section 5i shares bodies: acc[0] +=
// every gap squared, acc[1] += every (b - y) squared, a thread's elements in the order of dot_kernel<VEC>)
template <int VEC>
__device__ __forceinline__ void residual_gap_walk(const double *__restrict__ b, const double *__restrict__ y,
                                                  const double *__restrict__ r, int n, double *acc) {
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      const double2 bv = *reinterpret_cast<const double2 *>(b + i);
      const double2 yv = *reinterpret_cast<const double2 *>(y + i);
      const double2 rv = *reinterpret_cast<const double2 *>(r + i);
      const double tx = bv.x - yv.x, ty = bv.y - yv.y;
      const double gx = tx - rv.x, gy = ty - rv.y;
      acc[0] += gx * gx;
      acc[0] += gy * gy;
      acc[1] += tx * tx;
      acc[1] += ty * ty;
    } else {
      const double t = b[i] - y[i];
      const double g = t - r[i];
      acc[0] += g * g;
      acc[1] += t * t;
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void residual_gap_kernel(const double *__restrict__ b,
                                                                  const double *__restrict__ y,
                                                                  const double *__restrict__ r, int n,
                                                                  ReduceOutK out) {
  __shared__ double s_w[16];
  double acc[2] = {0.0, 0.0};
  residual_gap_walk<VEC>(b, y, r, n, acc);
  reduce_finish_k<2>(acc, out, s_w);
}

// residual_gap_kernel with the verdict formed where the sums are: the last arriver folds the block partials in its
// fixed order (the same two totals, bit for bit) and thread 0 leaves {gap2, tt2, verdict, queued events} in
// out.dev_out, device memory, with vector stores -- verdict 1.0 when gap2 <= limit and both sums are finite (the
// host's pass rule, context.py _check_passes, with limit = check_tol^2 ||b||^2 formed there: a NaN fails the
// comparison), else 2.0.  residual_guard_kernel behind it acts on the word.
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void residual_check_kernel(const double *__restrict__ b,
                                                                    const double *__restrict__ y,
                                                                    const double *__restrict__ r, int n, double limit,
                                                                    ReduceOutB out) {
  __shared__ double s_w[16];
  double acc[2] = {0.0, 0.0};
  residual_gap_walk<VEC>(b, y, r, n, acc);
  double tot[2];
  if (!reduce_totals_k<2>(acc, out, s_w, tot) || threadIdx.x != 0) return;
  const uint32_t nev = reduce_rearm(out);
  const bool ok = tot[0] <= limit && __builtin_isfinite(tot[0]) && __builtin_isfinite(tot[1]);
  out.dev_out[0] = tot[0];
  out.dev_out[1] = tot[1];
  out.dev_out[2] = ok ? 1.0 : 2.0;
  out.dev_out[3] = (double)nev;
}

// the check's verdict acted on: chk[2] == 1.0 (passed): x_ckpt <- x; anything else: x <- x_ckpt.  Every thread reads
// the word, which this kernel never writes: the decision is uniform over the grid and no workgroup waits for
// another.  Plain copies, never a 0 / 1 mask (0 * inf is NaN; copy_block_kernel); PAIRS: both 16-byte aligned.
template <bool PAIRS>
__global__ __launch_bounds__(ABFT_BLOCK) void residual_guard_kernel(double *x, double *x_ckpt,
                                                                    const double *__restrict__ chk, int n) {
  const bool passed = chk[2] == 1.0;
  double *dst = passed ? x_ckpt : x;
  const double *src = passed ? x : x_ckpt;
  const long stride = (long)gridDim.x * ABFT_BLOCK * 2;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * 2; i < n; i += stride) {
    if (i + 1 < n) {
      if (PAIRS) {
        *reinterpret_cast<double2 *>(dst + i) = *reinterpret_cast<const double2 *>(src + i);
      } else {
        const double s0 = src[i], s1 = src[i + 1];
        dst[i] = s0; dst[i + 1] = s1;
      }
    } else {
      dst[i] = src[i];
    }
  }
}

// r = b - y, p = r, and r.r. VEC is the element walk of dot_kernel<VEC> on r (the grid too:
// reduce_blocks(n)), so r.r is abft_hip_dot(r, r) bit for bit; PAIRS: every operand 16-byte
// aligned (VEC = 2 without it loads the pairs one by one, same order of additions).
template <int VEC, bool PAIRS>
__global__ __launch_bounds__(ABFT_BLOCK) void residual_restart_kernel(const double *__restrict__ b,
                                                                      const double *__restrict__ y,
                                                                      double *__restrict__ r, double *__restrict__ p,
                                                                      int n, ReduceOut out) {
  __shared__ double s_w[4];
  double acc = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 rv;
      if (PAIRS) {
        const double2 bv = *reinterpret_cast<const double2 *>(b + i);
        const double2 yv = *reinterpret_cast<const double2 *>(y + i);
        rv = make_double2(bv.x - yv.x, bv.y - yv.y);
        *reinterpret_cast<double2 *>(r + i) = rv;
        *reinterpret_cast<double2 *>(p + i) = rv;
      } else {
        rv = make_double2(b[i] - y[i], b[i + 1] - y[i + 1]);
        r[i] = rv.x; r[i + 1] = rv.y;
        p[i] = rv.x; p[i + 1] = rv.y;
      }
      acc += rv.x * rv.x;
      acc += rv.y * rv.y;
    } else {
      const double rs = b[i] - y[i];
      r[i] = rs;
      p[i] = rs;
      acc += rs * rs;
    }
  }
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// per column j: out[2j] = gap2, out[2j + 1] = tt2 as residual_gap_kernel forms them; 0 for a column
// whose bit is clear in `active`
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void residual_gap_block_kernel(const double *__restrict__ b,
                                                                        const double *__restrict__ y,
                                                                        const double *__restrict__ r, uint32_t active,
                                                                        int n, ReduceOutW out) {
  __shared__ double s_w[16 * K];
  double acc[2 * K];
#pragma unroll
  for (int j = 0; j < 2 * K; j++) acc[j] = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double bv[K], yv[K], rv[K];
    block_load<K>(b + i * K, bv);
    block_load<K>(y + i * K, yv);
    block_load<K>(r + i * K, rv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const bool on = (active >> j) & 1u;
      const double t = bv[j] - yv[j];
      const double g = t - rv[j];
      acc[2 * j] += on ? g * g : 0.0;
      acc[2 * j + 1] += on ? t * t : 0.0;
    }
  }
  reduce_finish_k<2 * K>(acc, out, s_w);
}

// R[:, j] = B[:, j] - Y[:, j], P[:, j] = R[:, j] for the columns set in `mask` (the others keep their
// bits); rr[j] = R[:, j] . R[:, j] for every column, in dot_block_kernel<K>'s shape
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void residual_restart_block_kernel(const double *__restrict__ b,
                                                                            const double *__restrict__ y,
                                                                            double *__restrict__ r,
                                                                            double *__restrict__ p, uint32_t mask,
                                                                            int n, ReduceOutK out) {
  __shared__ double s_w[8 * K];
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double bv[K], yv[K], rv[K], pv[K];
    block_load<K>(b + i * K, bv);
    block_load<K>(y + i * K, yv);
    block_load<K>(r + i * K, rv);
    block_load<K>(p + i * K, pv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const bool on = (mask >> j) & 1u;
      const double rs = bv[j] - yv[j];
      rv[j] = on ? rs : rv[j];
      pv[j] = on ? rs : pv[j];
      acc[j] += rv[j] * rv[j];
    }
    block_store<K>(r + i * K, rv);
    block_store<K>(p + i * K, pv);
  }
  reduce_finish_k<K>(acc, out, s_w);
}

// dst[:, j] = src[:, j] for the columns set in `mask` (a select: inf and NaN are copied as they are)
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void copy_block_kernel(double *__restrict__ dst,
                                                                const double *__restrict__ src, uint32_t mask,
                                                                int n) {
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double dv[K], sv[K];
    block_load<K>(dst + i * K, dv);
    block_load<K>(src + i * K, sv);
#pragma unroll
    for (int j = 0; j < K; j++) dv[j] = ((mask >> j) & 1u) ? sv[j] : dv[j];
    block_store<K>(dst + i * K, dv);
  }
}

hipError_t launch_flip_vector(double *v, unsigned long long mask, hipStream_t s) {
  hipLaunchKernelGGL(flip_vector_kernel, dim3(1), dim3(1), 0, s, v, mask);
  return hipGetLastError();
}

hipError_t launch_residual_gap(const double *b, const double *y, const double *r, int n, const ReduceOutK &out,
                               hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(residual_gap_kernel, (), aligned16(b, y, r), nb, b, y, r, n, out);
  return hipGetLastError();
}

// (grid and VEC exactly as launch_residual_gap chooses them: the two sums are its bits)
hipError_t launch_residual_check(const double *b, const double *y, const double *r, int n, double limit,
                                 const ReduceOutB &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(residual_check_kernel, (), aligned16(b, y, r), nb, b, y, r, n, limit, out);
  return hipGetLastError();
}

hipError_t launch_residual_guard(double *x, double *x_ckpt, const double *chk, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  if (aligned16(x, x_ckpt))
    hipLaunchKernelGGL(residual_guard_kernel<true>, dim3(nb), dim3(ABFT_BLOCK), 0, s, x, x_ckpt, chk, n);
  else
    hipLaunchKernelGGL(residual_guard_kernel<false>, dim3(nb), dim3(ABFT_BLOCK), 0, s, x, x_ckpt, chk, n);
  return hipGetLastError();
}

hipError_t launch_residual_restart(const double *b, const double *y, double *r, double *p, int n, const ReduceOut &out,
                                   hipStream_t s) {
  const int nb = reduce_blocks(n);
  if (!aligned16(r))  // launch_dot(r, r) would run dot_kernel<1>
    hipLaunchKernelGGL((residual_restart_kernel<1, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, b, y, r, p, n, out);
  else if (aligned16(b, y, p))
    hipLaunchKernelGGL((residual_restart_kernel<2, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, b, y, r, p, n, out);
  else
    hipLaunchKernelGGL((residual_restart_kernel<2, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, b, y, r, p, n, out);
  return hipGetLastError();
}

hipError_t launch_residual_gap_block(const double *b, const double *y, const double *r, int n, int k, uint32_t active,
                                     const ReduceOutW &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL(residual_gap_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, b, y, r, active, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_residual_restart_block(const double *b, const double *y, double *r, double *p, int n, int k,
                                         uint32_t mask, const ReduceOutK &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL(residual_restart_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, b, y, r, p, mask, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_copy_block(double *dst, const double *src, int n, int k, uint32_t mask, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) hipLaunchKernelGGL(copy_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, dst, src, mask, n)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// ---- Jacobi preconditioning: z = dinv * r, one rounded product formed in registers, never stored ----
// The preconditioned forms of the vector kernels above.  Each walks the vectors exactly as the kernel
// it stands in for (same grid reduce_blocks(n), same stride, VEC by the alignment of the SAME operands;
// PAIRS: dinv -- and p where it is only written -- are 16-byte aligned too, else their pairs move one
// entry at a time, same order of operations), and every reduction has that kernel's shape: per thread a
// serial sum, block_sum, the last block's fixed-order fold.  With dinv == 1.0 in every entry z is r bit
// for bit, so both sums are the bits the plain kernel returns.  Two sums per call, {sum r z, sum r r},
// through the K-wide slot as residual_gap_kernel returns its two.
template <bool PAIRS>
__device__ __forceinline__ double2 pair_load(const double *v, long i) {
  if (PAIRS) return *reinterpret_cast<const double2 *>(v + i);
  return make_double2(v[i], v[i + 1]);
}
template <bool PAIRS>
__device__ __forceinline__ void pair_store(double *v, long i, double2 t) {
  if (PAIRS) {
    *reinterpret_cast<double2 *>(v + i) = t;
  } else {
    v[i] = t.x; v[i + 1] = t.y;
  }
}

// p = z; {r.z, r.r}.  Walks r as dot_kernel<VEC> does on dot(r, r).
template <int VEC, bool PAIRS>
__global__ __launch_bounds__(ABFT_BLOCK) void precond_start_kernel(const double *__restrict__ r,
                                                                   const double *__restrict__ dinv,
                                                                   double *__restrict__ p, int n, ReduceOutK out) {
  __shared__ double s_w[16];
  double acc[2] = {0.0, 0.0};
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      const double2 rv = *reinterpret_cast<const double2 *>(r + i);
      const double2 dv = pair_load<PAIRS>(dinv, i);
      const double2 zv = make_double2(dv.x * rv.x, dv.y * rv.y);
      pair_store<PAIRS>(p, i, zv);
      acc[0] += rv.x * zv.x;
      acc[0] += rv.y * zv.y;
      acc[1] += rv.x * rv.x;
      acc[1] += rv.y * rv.y;
    } else {
      const double rs = r[i];
      const double z = dinv[i] * rs;
      p[i] = z;
      acc[0] += rs * z;
      acc[1] += rs * rs;
    }
  }
  reduce_finish_k<2>(acc, out, s_w);
}

// r -= alpha w; {r.z, r.r} of the new r added to acc.  XHALF = false walks as calc_r_kernel<VEC> does (x += alpha p
// is left to the calc_p_precond that follows), XHALF = true as calc_xr_kernel<VEC> with x += alpha p.  The one body
// of calc_xr_precond_kernel and, as its XHALF = false instance, of calc_r_precond_until_kernel.
// (x, r: no __restrict__ -- operands that alias each other take the XHALF form)
template <int VEC, bool PAIRS, bool XHALF>
__device__ __forceinline__ void calc_xr_precond_walk(double *x, double *r, const double *p, const double *w,
                                                     const double *__restrict__ dinv, double alpha, int n,
                                                     double *acc) {
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 rv = *reinterpret_cast<const double2 *>(r + i);
      const double2 wv = *reinterpret_cast<const double2 *>(w + i);
      const double2 dv = pair_load<PAIRS>(dinv, i);
      if (XHALF) {
        double2 xv = *reinterpret_cast<const double2 *>(x + i);
        const double2 pv = *reinterpret_cast<const double2 *>(p + i);
        xv.x += alpha * pv.x; xv.y += alpha * pv.y;
        *reinterpret_cast<double2 *>(x + i) = xv;
      }
      rv.x -= alpha * wv.x; rv.y -= alpha * wv.y;
      *reinterpret_cast<double2 *>(r + i) = rv;
      const double zx = dv.x * rv.x, zy = dv.y * rv.y;
      acc[0] += rv.x * zx;
      acc[0] += rv.y * zy;
      acc[1] += rv.x * rv.x;
      acc[1] += rv.y * rv.y;
    } else {
      const double d = dinv[i];
      const double rs = r[i] - alpha * w[i];
      if (XHALF) x[i] = x[i] + alpha * p[i];
      r[i] = rs;
      const double z = d * rs;
      acc[0] += rs * z;
      acc[1] += rs * rs;
    }
  }
}

template <int VEC, bool PAIRS, bool XHALF>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_xr_precond_kernel(double *x, double *r, const double *p,
                                                                     const double *w,
                                                                     const double *__restrict__ dinv, double alpha,
                                                                     int n, ReduceOutK out) {
  __shared__ double s_w[16];
  double acc[2] = {0.0, 0.0};
  calc_xr_precond_walk<VEC, PAIRS, XHALF>(x, r, p, w, dinv, alpha, n, acc);
  reduce_finish_k<2>(acc, out, s_w);
}

// p = z + beta p, z recomputed from the operands calc_xr_precond multiplied (the same bits).  XHALF:
// with the x += alpha p the preceding calc_xr_precond left behind, walking as calc_px_kernel<VEC> does
// (p as calc_xr saw it); else as calc_p_kernel<VEC>.  The one body of calc_p_precond_kernel and, as its
// XHALF = true instance, of calc_px_precond_until_kernel.
template <int VEC, bool PAIRS, bool XHALF>
__device__ __forceinline__ void calc_p_precond_walk(double *__restrict__ p, const double *__restrict__ r,
                                                    const double *__restrict__ dinv, double *__restrict__ x,
                                                    double beta, double alpha, int n) {
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 pv = *reinterpret_cast<const double2 *>(p + i);
      const double2 rv = *reinterpret_cast<const double2 *>(r + i);
      const double2 dv = pair_load<PAIRS>(dinv, i);
      if (XHALF) {
        double2 xv = *reinterpret_cast<const double2 *>(x + i);
        xv.x += alpha * pv.x; xv.y += alpha * pv.y;
        *reinterpret_cast<double2 *>(x + i) = xv;
      }
      const double zx = dv.x * rv.x, zy = dv.y * rv.y;
      pv.x = zx + beta * pv.x;
      pv.y = zy + beta * pv.y;
      *reinterpret_cast<double2 *>(p + i) = pv;
    } else {
      const double ps = p[i];
      const double z = dinv[i] * r[i];
      if (XHALF) x[i] = x[i] + alpha * ps;
      p[i] = z + beta * ps;
    }
  }
}

template <int VEC, bool PAIRS, bool XHALF>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_p_precond_kernel(double *__restrict__ p,
                                                                    const double *__restrict__ r,
                                                                    const double *__restrict__ dinv,
                                                                    double *__restrict__ x, double beta, double alpha,
                                                                    int n) {
  calc_p_precond_walk<VEC, PAIRS, XHALF>(p, r, dinv, x, beta, alpha, n);
}

// VEC and PAIRS of one launch: `vec2` the alignment test of the plain kernel's operands, `pairs` that of the rest
// (MORE: the kernel's template arguments after VEC and PAIRS, in parentheses: `(, true)` / `(, false)` for XHALF, `()`
// for the guarded kernels, which have none)
#define ABFT_PRECOND_DISPATCH(KERNEL, MORE, ...)                                                            \
  do {                                                                                                      \
    if (!vec2)                                                                                              \
      hipLaunchKernelGGL((KERNEL<1, false ABFT_UNPAREN MORE>), dim3(nb), dim3(ABFT_BLOCK), 0, s, __VA_ARGS__);            \
    else if (pairs)                                                                                         \
      hipLaunchKernelGGL((KERNEL<2, true ABFT_UNPAREN MORE>), dim3(nb), dim3(ABFT_BLOCK), 0, s, __VA_ARGS__);             \
    else                                                                                                    \
      hipLaunchKernelGGL((KERNEL<2, false ABFT_UNPAREN MORE>), dim3(nb), dim3(ABFT_BLOCK), 0, s, __VA_ARGS__);            \
  } while (0)

hipError_t launch_precond_start(const double *r, const double *dinv, double *p, int n, const ReduceOutK &out,
                                hipStream_t s) {
  const int nb = reduce_blocks(n);
  if (!aligned16(r))  // launch_dot(r, r) would run dot_kernel<1>
    hipLaunchKernelGGL((precond_start_kernel<1, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, dinv, p, n, out);
  else if (aligned16(dinv, p))
    hipLaunchKernelGGL((precond_start_kernel<2, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, dinv, p, n, out);
  else
    hipLaunchKernelGGL((precond_start_kernel<2, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, dinv, p, n, out);
  return hipGetLastError();
}

// x == nullptr: the r half alone (launch_calc_r's walk), else launch_calc_xr's
hipError_t launch_calc_xr_precond(double *x, double *r, const double *p, const double *w, const double *dinv,
                                  double alpha, int n, const ReduceOutK &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
  const bool pairs = aligned16(dinv);
  if (x) {
    const bool vec2 = aligned16(x, r, p, w);
    ABFT_PRECOND_DISPATCH(calc_xr_precond_kernel, (, true), x, r, p, w, dinv, alpha, n, out);
  } else {
    const bool vec2 = aligned16(r, w);
    ABFT_PRECOND_DISPATCH(calc_xr_precond_kernel, (, false), x, r, p, w, dinv, alpha, n, out);
  }
  return hipGetLastError();
}

// x == nullptr: p = z + beta p alone (launch_calc_p's walk), else with x += alpha p (launch_calc_px's)
hipError_t launch_calc_p_precond(double *p, const double *r, const double *dinv, double *x, double beta, double alpha,
                                 int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  const bool pairs = aligned16(dinv);
  if (x) {
    const bool vec2 = aligned16(p, r, x);
    ABFT_PRECOND_DISPATCH(calc_p_precond_kernel, (, true), p, r, dinv, x, beta, alpha, n);
  } else {
    const bool vec2 = aligned16(p, r);
    ABFT_PRECOND_DISPATCH(calc_p_precond_kernel, (, false), p, r, dinv, x, beta, alpha, n);
  }
  return hipGetLastError();
}

// ---- the guarded preconditioned iteration (abft_hip_pcg_iteration_until_dev) ----
// calc_xr_precond_kernel<VEC, PAIRS, false> and calc_p_precond_kernel<VEC, PAIRS, true> behind the stop test, records
// of the GuardQuad shape (guard_protocol.h); the walk, the per-thread sums and the fold of a live launch are those
// kernels', bit for bit.
// (Symbols of their own, as the plain guarded pair; the streaming loops are calc_xr_precond_walk<.., false> and
// calc_p_precond_walk<.., true>, and the sums meet through reduce_totals_k as the unguarded kernel's do.)
template <int VEC, bool PAIRS>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_precond_until_kernel(double *r, const double *w,
                                                                          const double *__restrict__ dinv,
                                                                          const double *in, const double *pw,
                                                                          double threshold, double *alpha_out, int n,
                                                                          ReduceOutD out) {
  __shared__ double s_w[16];
  double alpha;
  if (!guard_r_head<GuardQuad>(in, pw, threshold, alpha_out, out, &alpha)) return;
  double acc[2] = {0.0, 0.0};
  calc_xr_precond_walk<VEC, PAIRS, false>(nullptr, r, nullptr, w, dinv, alpha, n, acc);
  reduce_finish_d(acc, out, s_w);
}

template <int VEC, bool PAIRS>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_precond_until_kernel(double *__restrict__ p,
                                                                           const double *__restrict__ r,
                                                                           const double *__restrict__ dinv,
                                                                           double *__restrict__ x, const double *in,
                                                                           const double *out, double threshold,
                                                                           const double *alpha_ptr, int n) {
  if (!GuardQuad::live(in, threshold)) return;
  const double beta = GuardQuad::beta(in, out);
  const double alpha = *alpha_ptr;
  calc_p_precond_walk<VEC, PAIRS, true>(p, r, dinv, x, beta, alpha, n);
}

// VEC and PAIRS as launch_calc_xr_precond(x == nullptr) and launch_calc_p_precond(x != nullptr) choose them:
// the sums are added in the same order
hipError_t launch_calc_r_precond_until(double *r, const double *w, const double *dinv, const double *in,
                                       const double *pw, double threshold, double *alpha_out, int n,
                                       const ReduceOutD &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
  const bool vec2 = aligned16(r, w), pairs = aligned16(dinv);
  ABFT_PRECOND_DISPATCH(calc_r_precond_until_kernel, (), r, w, dinv, in, pw, threshold, alpha_out, n, out);
  return hipGetLastError();
}

hipError_t launch_calc_px_precond_until(double *p, const double *r, const double *dinv, double *x, const double *in,
                                        const double *out, double threshold, const double *alpha_ptr, int n,
                                        hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  const bool vec2 = aligned16(p, r, x), pairs = aligned16(dinv);
  ABFT_PRECOND_DISPATCH(calc_px_precond_until_kernel, (), p, r, dinv, x, in, out, threshold, alpha_ptr, n);
  return hipGetLastError();
}

// Block forms: one thread per row over the K columns, as the block kernels above; dinv[i] is loaded
// once per row (one operator for all columns).  A column whose bit is clear keeps its bits (a
// select).  Sums in dot_block_kernel<K>'s shape, value 2j = column j's r.z, 2j + 1 its r.r, for every
// column, through the 2K-wide slot.
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void precond_start_block_kernel(const double *__restrict__ r,
                                                                         const double *__restrict__ dinv,
                                                                         double *__restrict__ p, uint32_t mask, int n,
                                                                         ReduceOutW out) {
  __shared__ double s_w[16 * K];
  double acc[2 * K];
#pragma unroll
  for (int j = 0; j < 2 * K; j++) acc[j] = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double rv[K], pv[K];
    const double d = dinv[i];
    block_load<K>(r + i * K, rv);
    block_load<K>(p + i * K, pv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const double z = d * rv[j];
      pv[j] = ((mask >> j) & 1u) ? z : pv[j];
      acc[2 * j] += rv[j] * z;
      acc[2 * j + 1] += rv[j] * rv[j];
    }
    block_store<K>(p + i * K, pv);
  }
  reduce_finish_k<2 * K>(acc, out, s_w);
}

template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_xr_precond_block_kernel(double *__restrict__ x,
                                                                           double *__restrict__ r,
                                                                           const double *__restrict__ p,
                                                                           const double *__restrict__ w,
                                                                           const double *__restrict__ dinv,
                                                                           BlockScalars alpha, uint32_t active, int n,
                                                                           ReduceOutW out) {
  __shared__ double s_w[16 * K];
  double acc[2 * K];
#pragma unroll
  for (int j = 0; j < 2 * K; j++) acc[j] = 0.0;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double xv[K], rv[K], pv[K], wv[K];
    const double d = dinv[i];
    block_load<K>(x + i * K, xv);
    block_load<K>(r + i * K, rv);
    block_load<K>(p + i * K, pv);
    block_load<K>(w + i * K, wv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const bool on = (active >> j) & 1u;
      const double xs = xv[j] + alpha.v[j] * pv[j];  // calc_xr_block_kernel's two roundings
      const double rs = rv[j] - alpha.v[j] * wv[j];
      xv[j] = on ? xs : xv[j];
      rv[j] = on ? rs : rv[j];
      const double z = d * rv[j];
      acc[2 * j] += rv[j] * z;
      acc[2 * j + 1] += rv[j] * rv[j];
    }
    block_store<K>(x + i * K, xv);
    block_store<K>(r + i * K, rv);
  }
  reduce_finish_k<2 * K>(acc, out, s_w);
}

template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_p_precond_block_kernel(double *__restrict__ p,
                                                                          const double *__restrict__ r,
                                                                          const double *__restrict__ dinv,
                                                                          BlockScalars beta, uint32_t active, int n) {
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double pv[K], rv[K];
    const double d = dinv[i];
    block_load<K>(p + i * K, pv);
    block_load<K>(r + i * K, rv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const double z = d * rv[j];
      const double ps = z + beta.v[j] * pv[j];
      pv[j] = ((active >> j) & 1u) ? ps : pv[j];
    }
    block_store<K>(p + i * K, pv);
  }
}

hipError_t launch_precond_start_block(const double *r, const double *dinv, double *p, int n, int k, uint32_t mask,
                                      const ReduceOutW &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL(precond_start_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, r, dinv, p, mask, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_xr_precond_block(double *x, double *r, const double *p, const double *w, const double *dinv,
                                        int n, int k, const BlockScalars &alpha, uint32_t active, const ReduceOutW &out,
                                        hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                                  \
  hipLaunchKernelGGL(calc_xr_precond_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, x, r, p, w, dinv, alpha, active, \
                     n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_p_precond_block(double *p, const double *r, const double *dinv, int n, int k,
                                       const BlockScalars &beta, uint32_t active, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL(calc_p_precond_block_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, p, r, dinv, beta, active, n)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// ---- the fused block iteration (abft_hip_spmm_dot, abft_hip_calc_r_block, abft_hip_calc_px_block) ----
// Fold of the K * nblk partials spmm_csr_kernel<.., DOT> left (column j's at parts + j * n): fold_partials_kernel's
// shape per column -- every workgroup adds a contiguous chunk in a fixed order -- and the chunk sums meet through
// reduce_finish_k, which publishes the K totals in the K-wide pinned slot.
// (fold_chunk_sum: the chunk sums, written once for spmm_fold_kernel, spmm_fold_dev_kernel and fold_partials_kernel)
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void spmm_fold_kernel(const double *__restrict__ parts, uint32_t n,
                                                               uint32_t chunk, ReduceOutK out) {
  __shared__ double s_w[8 * K];
  const uint32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = fold_chunk_sum(parts + (size_t)j * n, lo, hi);
  reduce_finish_k<K>(acc, out, s_w);
}

hipError_t launch_spmm_fold(const double *parts, uint32_t nblk, int k, const ReduceOutK &out, hipStream_t s) {
  uint32_t chunk;
  const uint32_t nb = fold_grid(nblk, &chunk);
#define ABFT_OP(K) hipLaunchKernelGGL(spmm_fold_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, parts, nblk, chunk, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// The r half of calc_xr_block_kernel / calc_xr_precond_block_kernel alone: the same grid, walk, operations
// and reduction, so with the same alpha and mask R and the sums are theirs bit for bit.  Reads r, w (dinv),
// writes r.
template <bool PRECOND> struct BlockSumsOut { typedef ReduceOutK type; };
template <> struct BlockSumsOut<true> { typedef ReduceOutW type; };

// (calc_r_block_walk: the one body of calc_r_block_kernel and calc_r_block_until_kernel.  alpha: K scalars, the
// kernel argument's array or the guarded kernel's own)
template <int K, bool PRECOND>
__device__ __forceinline__ void calc_r_block_walk(double *__restrict__ r, const double *__restrict__ w,
                                                  const double *__restrict__ dinv, const double *alpha,
                                                  uint32_t active, int n, double *acc) {
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double rv[K], wv[K];
    const double d = PRECOND ? dinv[i] : 0.0;
    block_load<K>(r + i * K, rv);
    block_load<K>(w + i * K, wv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const double rs = rv[j] - alpha[j] * wv[j];  // calc_xr_block_kernel's two roundings
      rv[j] = ((active >> j) & 1u) ? rs : rv[j];
      if (PRECOND) {
        const double z = d * rv[j];
        acc[2 * j] += rv[j] * z;
        acc[2 * j + 1] += rv[j] * rv[j];
      } else {
        acc[j] += rv[j] * rv[j];
      }
    }
    block_store<K>(r + i * K, rv);
  }
}

template <int K, bool PRECOND>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_block_kernel(double *__restrict__ r, const double *__restrict__ w,
                                                                  const double *__restrict__ dinv, BlockScalars alpha,
                                                                  uint32_t active, int n,
                                                                  typename BlockSumsOut<PRECOND>::type out) {
  constexpr int S = PRECOND ? 2 * K : K;
  __shared__ double s_w[8 * S];
  double acc[S];
#pragma unroll
  for (int j = 0; j < S; j++) acc[j] = 0.0;
  calc_r_block_walk<K, PRECOND>(r, w, dinv, alpha.v, active, n, acc);
  reduce_finish_k<S>(acc, out, s_w);
}

// x += alpha p and p = r + beta p (PRECOND: p = dinv * r + beta p) in one pass, p read once: the x half of
// calc_xr_block_kernel and calc_p_block_kernel (or their precond forms), the same operands and roundings.
// (calc_px_block_walk: the one body of calc_px_block_kernel and calc_px_block_until_kernel)
template <int K, bool PRECOND>
__device__ __forceinline__ void calc_px_block_walk(double *__restrict__ x, double *__restrict__ p,
                                                   const double *__restrict__ r, const double *__restrict__ dinv,
                                                   const double *alpha, const double *beta, uint32_t active, int n) {
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  for (long i = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n; i += stride) {
    double xv[K], pv[K], rv[K];
    const double d = PRECOND ? dinv[i] : 0.0;
    block_load<K>(x + i * K, xv);
    block_load<K>(p + i * K, pv);
    block_load<K>(r + i * K, rv);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const bool on = (active >> j) & 1u;
      const double xs = xv[j] + alpha[j] * pv[j];
      const double z = PRECOND ? d * rv[j] : rv[j];
      const double ps = z + beta[j] * pv[j];
      xv[j] = on ? xs : xv[j];
      pv[j] = on ? ps : pv[j];
    }
    block_store<K>(x + i * K, xv);
    block_store<K>(p + i * K, pv);
  }
}

template <int K, bool PRECOND>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_block_kernel(double *__restrict__ x, double *__restrict__ p,
                                                                   const double *__restrict__ r,
                                                                   const double *__restrict__ dinv, BlockScalars alpha,
                                                                   BlockScalars beta, uint32_t active, int n) {
  calc_px_block_walk<K, PRECOND>(x, p, r, dinv, alpha.v, beta.v, active, n);
}

hipError_t launch_calc_r_block(double *r, const double *w, int n, int k, const BlockScalars &alpha, uint32_t active,
                               const ReduceOutK &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                               \
  hipLaunchKernelGGL((calc_r_block_kernel<K, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, (const double *)nullptr, \
                     alpha, active, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_r_precond_block(double *r, const double *w, const double *dinv, int n, int k,
                                       const BlockScalars &alpha, uint32_t active, const ReduceOutW &out,
                                       hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL((calc_r_block_kernel<K, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, dinv, alpha, active, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_px_block(double *x, double *p, const double *r, const double *dinv, int n, int k,
                                const BlockScalars &alpha, const BlockScalars &beta, uint32_t active, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                                  \
  if (dinv)                                                                                                         \
    hipLaunchKernelGGL((calc_px_block_kernel<K, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, dinv, alpha, beta, \
                       active, n);                                                                                  \
  else                                                                                                              \
    hipLaunchKernelGGL((calc_px_block_kernel<K, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, dinv, alpha, beta, \
                       active, n)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// ---- the guarded block iteration (abft_hip_cg_block_iteration_until_dev) ----
// spmm_fold_kernel<K>, calc_r_block_kernel<K, PRECOND> and calc_px_block_kernel<K, PRECOND> with their scalars on the
// device and the column mask decided there, on GuardBlock<K> records (guard_protocol.h).  A live column's walk, selects,
// sums and folds are those kernels', bit for bit; a frozen column keeps its bits through the same selects.
// (Symbols of their own, as the single guarded pairs; the chunk sums are fold_chunk_sum, the streaming loops
// calc_r_block_walk / calc_px_block_walk, and the sums meet through reduce_totals_k as the unguarded kernels' do.)

// spmm_fold_kernel<K> leaving {K totals, queued events} in dev_pw instead of the pinned slot
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void spmm_fold_dev_kernel(const double *__restrict__ parts, uint32_t n,
                                                                   uint32_t chunk, ReduceOutB out) {
  __shared__ double s_w[8 * K];
  const uint32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = fold_chunk_sum(parts + (size_t)j * n, lo, hi);
  reduce_finish_b<K>(acc, out, s_w);
}

hipError_t launch_spmm_fold_dev(const double *parts, uint32_t nblk, int k, const ReduceOutB &out, hipStream_t s) {
  uint32_t chunk;
  const uint32_t nb = fold_grid(nblk, &chunk);  // launch_spmm_fold's grid and chunks
#define ABFT_OP(K) hipLaunchKernelGGL(spmm_fold_dev_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, parts, nblk, chunk, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// a wave-uniform double moved into scalar registers (the same bits): a scalar formed by vector arithmetic from device
// words then costs the streaming loops no vector registers, as a kernel argument costs none
__device__ __forceinline__ double uniform_f64(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// The r half of every guarded block iteration is head, walk, tail.  The head -> the mask; none live: 0, the record
// handed on by one thread; else the K alphas, which one thread leaves in alpha_out for the x / p half.
// (noescape: the compiler passes the walk its alphas by value, as the unguarded kernel's code has them, only when it
// sees that no call kept the array's address -- and it decides before this head is inlined)
template <int K>
__device__ __forceinline__ uint32_t guard_block_r_head(const double *in, const double *pw, double threshold,
                                                       double *alpha_out, const ReduceOutB &out,
                                                       double *alpha __attribute__((noescape))) {
  const uint32_t active = GuardBlock<K>::live_mask(in, threshold);
  if (!active) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      GuardBlock<K>::hand_on(in, out.dev_out, __hip_atomic_load(out.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return 0u;
  }
#pragma unroll
  for (int j = 0; j < K; j++) alpha[j] = uniform_f64(GuardBlock<K>::alpha(in, pw, j));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < K; j++) alpha_out[j] = alpha[j];
  }
  return active;
}

// The tail: the S = PRECOND ? 2K : K sums meet (s_w: 8 S doubles) and the last block's first thread publishes
template <int K, bool PRECOND>
__device__ __forceinline__ void guard_block_r_tail(const double *acc, uint32_t active, const double *in,
                                                   const ReduceOutB &out, double *s_w) {
  constexpr int S = PRECOND ? 2 * K : K;
  double tot[S];
  if (!reduce_totals_k<S, ReduceOutB, uint32_t>(acc, out, s_w, tot) || threadIdx.x != 0) return;
  GuardBlock<K>::template publish<PRECOND>(tot, active, in, out.dev_out, reduce_rearm(out));
}

// The head of the x / p half -> the mask, and when it is not 0 the K alphas and betas (out: what the r half left)
template <int K>
__device__ __forceinline__ uint32_t guard_block_px_head(const double *in, const double *out, double threshold,
                                                        const double *alpha_ptr, double *alpha, double *beta) {
  const uint32_t active = GuardBlock<K>::live_mask(in, threshold);
  if (!active) return 0u;
#pragma unroll
  for (int j = 0; j < K; j++) {
    alpha[j] = alpha_ptr[j];
    beta[j] = uniform_f64(GuardBlock<K>::beta(in, out, j));
  }
  return active;
}

template <int K, bool PRECOND>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_block_until_kernel(double *__restrict__ r,
                                                                        const double *__restrict__ w,
                                                                        const double *__restrict__ dinv,
                                                                        const double *in, const double *pw,
                                                                        double threshold, double *alpha_out, int n,
                                                                        ReduceOutB out) {
  constexpr int S = PRECOND ? 2 * K : K;
  __shared__ double s_w[8 * S];
  double alpha[K], acc[S] = {};
  const uint32_t active = guard_block_r_head<K>(in, pw, threshold, alpha_out, out, alpha);
  if (!active) return;
  calc_r_block_walk<K, PRECOND>(r, w, dinv, alpha, active, n, acc);
  guard_block_r_tail<K, PRECOND>(acc, active, in, out, s_w);
}

template <int K, bool PRECOND>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_block_until_kernel(double *__restrict__ x, double *__restrict__ p,
                                                                         const double *__restrict__ r,
                                                                         const double *__restrict__ dinv,
                                                                         const double *in, const double *out,
                                                                         double threshold, const double *alpha_ptr,
                                                                         int n) {
  double alpha[K], beta[K];
  const uint32_t active = guard_block_px_head<K>(in, out, threshold, alpha_ptr, alpha, beta);
  if (!active) return;
  calc_px_block_walk<K, PRECOND>(x, p, r, dinv, alpha, beta, active, n);
}

hipError_t launch_calc_r_block_until(double *r, const double *w, const double *dinv, const double *in,
                                     const double *pw, double threshold, double *alpha_out, int n, int k,
                                     const ReduceOutB &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                                    \
  if (dinv)                                                                                                           \
    hipLaunchKernelGGL((calc_r_block_until_kernel<K, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, dinv, in, pw,    \
                       threshold, alpha_out, n, out);                                                                 \
  else                                                                                                                \
    hipLaunchKernelGGL((calc_r_block_until_kernel<K, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, dinv, in, pw,   \
                       threshold, alpha_out, n, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_px_block_until(double *x, double *p, const double *r, const double *dinv, const double *in,
                                      const double *out, double threshold, const double *alpha_ptr, int n, int k,
                                      hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                                    \
  if (dinv)                                                                                                           \
    hipLaunchKernelGGL((calc_px_block_until_kernel<K, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, dinv, in,    \
                       out, threshold, alpha_ptr, n);                                                                 \
  else                                                                                                                \
    hipLaunchKernelGGL((calc_px_block_until_kernel<K, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, dinv, in,   \
                       out, threshold, alpha_ptr, n)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// ---- the inverse diagonal (abft_hip_matrix_diag_inverse) over the stored arrays ----
// d = the sum, in storage order, of the values of a row's (COO: an output group's) elements that sit on
// the diagonal; in these two layouts storage order inside a row / group is the caller's.  The column is
// the stored word under `colmask` (the ECC byte off in the ECC modes, as the SpMV reads it); nothing is
// checked or repaired here.  Element ranges are clamped to nnz: a damaged row pointer must not send a
// read outside the arrays.  No usable diagonal (none stored: d = 0; not finite; <= 0): 1.0, counted.
__device__ __forceinline__ double diag_invert(double d, uint32_t *bad) {
  if (d > 0.0 && d <= 1.7976931348623157e308) return 1.0 / d;
  atomicAdd(bad, 1u);
  return 1.0;
}

__global__ __launch_bounds__(ABFT_BLOCK) void diag_csr_kernel(const uint32_t *__restrict__ rowptr,
                                                              const uint32_t *__restrict__ cols,
                                                              const double *__restrict__ vals, uint32_t n, uint32_t nnz,
                                                              uint32_t colmask, double *__restrict__ dinv,
                                                              uint32_t *bad) {
  for (uint32_t row = blockIdx.x * ABFT_BLOCK + threadIdx.x; row < n; row += gridDim.x * ABFT_BLOCK) {
    const uint32_t hi = min(rowptr[row + 1], nnz), lo = min(rowptr[row], hi);
    double d = 0.0;
    for (uint32_t e = lo; e < hi; e++)
      if ((cols[e] & colmask) == row) d += vals[e];
    dinv[row] = diag_invert(d, bad);
  }
}

__global__ __launch_bounds__(ABFT_BLOCK) void diag_coo_kernel(const uint32_t *__restrict__ grp_ptr,
                                                              const uint4 *__restrict__ elems, uint32_t n, uint32_t nnz,
                                                              uint32_t colmask, double *__restrict__ dinv,
                                                              uint32_t *bad) {
  for (uint32_t c = blockIdx.x * ABFT_BLOCK + threadIdx.x; c < n; c += gridDim.x * ABFT_BLOCK) {
    const uint32_t hi = min(grp_ptr[c + 1], nnz), lo = min(grp_ptr[c], hi);
    double d = 0.0;
    for (uint32_t e = lo; e < hi; e++) {
      const uint4 el = elems[e];
      if ((el.x & colmask) == c && el.y == c) d += as_double(el.z, el.w);
    }
    dinv[c] = diag_invert(d, bad);
  }
}

hipError_t launch_diag_csr(const CsrDev &A, uint32_t colmask, double *dinv, uint32_t *bad, hipStream_t s) {
  if (!A.n_out) return hipSuccess;
  const int nb = reduce_blocks((int)A.n_out);
  hipLaunchKernelGGL(diag_csr_kernel, dim3(nb), dim3(ABFT_BLOCK), 0, s, A.rowptr, A.cols, A.vals, A.n_out, A.nnz,
                     colmask, dinv, bad);
  return hipGetLastError();
}

hipError_t launch_diag_coo(const CooDev &A, uint32_t colmask, double *dinv, uint32_t *bad, hipStream_t s) {
  if (!A.n_out) return hipSuccess;
  const int nb = reduce_blocks((int)A.n_out);
  hipLaunchKernelGGL(diag_coo_kernel, dim3(nb), dim3(ABFT_BLOCK), 0, s, A.grp_ptr, A.elems, A.n_out, A.nnz, colmask,
                     dinv, bad);
  return hipGetLastError();
}

// ---- the tail of a CG iteration in ONE launch (fixed-iteration loop, scalars on the device) ----
// Behind the SpMV the loop of cg.cpp:100-112 runs three small kernels -- the fold of the fused p.w partials,
// calc_r (r -= alpha w, r.r), calc_px (x += alpha p, p = r + beta p) -- each ending in a reduction and, across
// ranks, a board all-reduce.  On a 1/8 shard of configs[3] they move 3 us worth of bytes in 22-26 us: launch
// boundaries and reduction tails.  cg_tail_kernel is the three in one launch of co-resident workgroups with two
// grid-wide hand-offs (a flag the other workgroups poll):
//   A  workgroup 0 folds the SpMV's partials (after the COO fix-up, if any), all-reduces {p.w, events} over the
//      board and publishes it; every workgroup then forms alpha = rr / p.w
//   B  r -= alpha w and the block partials of r.r; the workgroup that arrives last folds them, all-reduces
//      {r.r, events} and publishes; every workgroup then forms beta = rr_new / rr
//   C  x += alpha p; p = r + beta p
// Same bits as the three kernels: 1024-thread workgroups stand for four "virtual" 256-thread blocks each (a
// quarter = 4 waves with its own LDS slots), the virtual blocks walk the vectors exactly as calc_r_kernel /
// calc_px_kernel blocks do on a grid of reduce_blocks(n), every fold keeps its shape (fuse_finalize_kernel's
// 1024-thread fold, or fold_partials_kernel's chunks for many partials; reduce_finish's fold of the block
// partials), and alpha and beta are the same IEEE quotients.  Every wait is bounded (a launch whose workgroups
// are all resident never waits long; should one ever give up, the scalars become NaN -- loud, not wrong).
__device__ __forceinline__ double quarter_sum(double v, double *s_w) {  // block_sum for each quarter of 1024 threads
  v = wave_sum(v);
  if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t q4 = (threadIdx.x >> 8) * 4u;
  return (s_w[q4] + s_w[q4 + 1u]) + (s_w[q4 + 2u] + s_w[q4 + 3u]);
}

// The hand-off words of cg_tail_kernel never go back: every launch reads, from `base`, the values the previous launch
// left its counters and flags at, and waits for them to have GROWN by its own amounts (nothing to reset at the end,
// no exit counter); workgroup 0 leaves the next launch's bases.  Layout of TailArgs::sync (64-bit words):
//   [0..7]   arrivals of phase B, sharded by blockIdx & 7 (an atomic on one address retires one add per ~12 ns)
//   [8]      arrivals of the chunk fold        [9] flag A (generation)        [10] flag B (generation)
//   [12]     arrivals of phase B in one counter (host-memory board: ONE workgroup folds, the last to arrive)
//   [16..23] base of [0..7] for this launch    [24] base of [8]    [25] generation of the previous launch    [27] base of [12]
__device__ __forceinline__ bool tail_wait_ge64(unsigned long long *sync, uint32_t at, unsigned long long want, unsigned long long ticks) {
  const unsigned long long t0 = (unsigned long long)wall_clock64();
  while (__hip_atomic_load(sync + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
    if ((unsigned long long)wall_clock64() - t0 > ticks) {
      __hip_atomic_store(sync + 30, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sticky: see cg_tail_kernel
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return true;
}

// all eight shards of the phase-B arrival counter have reached this launch's targets (the shards share one 64-byte
// line); `want`: read from the bases BEFORE this workgroup's own arrival -- workgroup 0 rewrites the bases at its end
__device__ __forceinline__ bool tail_wait_arrivals(unsigned long long *sync, const unsigned long long *want,
                                                   unsigned long long ticks) {
  const unsigned long long t0 = (unsigned long long)wall_clock64();
  for (;;) {
    // (the eight words in four 16-byte loads that are in flight together: one trip to memory per look, not eight)
    u64x2 c0, c1, c2, c3;
    sys_load4_b128(reinterpret_cast<const u64x2 *>(sync), reinterpret_cast<const u64x2 *>(sync + 2),
                   reinterpret_cast<const u64x2 *>(sync + 4), reinterpret_cast<const u64x2 *>(sync + 6), c0, c1, c2, c3);
    if (c0.x >= want[0] && c0.y >= want[1] && c1.x >= want[2] && c1.y >= want[3] && c2.x >= want[4] && c2.y >= want[5] &&
        c3.x >= want[6] && c3.y >= want[7])
      return true;
    if ((unsigned long long)wall_clock64() - t0 > ticks) {
      __hip_atomic_store(sync + 30, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// FAST (host: every workgroup owns exactly four virtual blocks and a thread's chain is at most four pairs, i.e. n <= 2^22
// and nothing is looped over): the elements stay in registers from phase B to phase C, and the loads of a phase are
// issued BEFORE the hand-off in front of it -- r and w before p.w is known, p and x before r.r is.
#ifdef ABFT_DBG_STAMPS
#define TSTAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) a.sync[40 + (k)] = (unsigned long long)wall_clock64(); } while (0)
#else
#define TSTAMP(k)
#endif
// Q: virtual 256-thread blocks per workgroup (4, 2 or 1: workgroups of 1024, 512 or 256 threads).  The host picks 4;
// the smaller ones (more workgroups for mid-size vectors, more arrivals per grid-wide point) measured slower.
template <int VEC, bool FAST, int Q>
__global__ __launch_bounds__(256 * Q) void cg_tail_kernel(TailArgs a) {
  __shared__ double s_w[16];
  __shared__ double s_scal;
  __shared__ uint32_t s_last;
  const uint32_t t = threadIdx.x, q = t >> 8, tq = t & 255u;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  unsigned long long *sync = a.sync;
  TSTAMP(0);
  // (these scalars are only needed later: their loads run beside everything up to there instead of in front of it)
  const double rr = *a.rr;
  const uint32_t nev_a = __hip_atomic_load(a.f.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long gen = sync[25] + 1ull;  // (plain loads of what the previous launch left: visible at a kernel boundary)
  // the board's sequence number as the previous launch left it: this launch's all-reduces are seq0 + 1 and + 2
  const unsigned long long seq0 = a.f.peers.size ? *a.f.peers.counter : 0ull;
  // A hand-off through memory costs a few microseconds (the L2s of the XCDs meet in memory), so wherever the input
  // of a fold is small EVERY workgroup folds it for itself instead of waiting for one that does: the SpMV's partials
  // (unless there are thousands of them, or the COO fix-up has to run first), the block partials of r.r, and -- with
  // the board in device memory -- the ranks' slots, which every workgroup reads from this rank's own copy while
  // workgroup 0 alone publishes.  Same folds, same order: same bits in every workgroup.
  const bool each_a = !a.fx.on && !a.fold_nb && (a.f.peers.size == 0 || a.f.peers.boards != nullptr);
  const bool each_b = a.o.peers.size == 0 || a.o.peers.boards != nullptr;
  const long stride = (long)a.nbv * ABFT_BLOCK * VEC;

  // FAST: this thread's (at most four) pairs of r and w, on their way while p.w is being folded
  constexpr int NK = FAST ? 4 : 1;
  double2 rv[NK], wv[NK], pv[NK], xv[NK];
  const uint32_t myvb = blockIdx.x * (uint32_t)Q + q;
  const long i0 = ((long)myvb * ABFT_BLOCK + tq) * 2;
  if (FAST) {
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const long i = i0 + (long)k * stride;
      rv[k] = wv[k] = make_double2(0.0, 0.0);
      if (myvb < a.nbv && i + 1 < a.n) {
        rv[k] = *reinterpret_cast<const double2 *>(a.r + i);
        wv[k] = *reinterpret_cast<const double2 *>(a.w + i);
      } else if (myvb < a.nbv && i < a.n) {  // the vector's odd last element
        rv[k].x = a.r[i];
        wv[k].x = a.w[i];
      }
    }
  }

  TSTAMP(1);
  // ---- A: p.w ----
  if (a.fx.on && blockIdx.x == 0) {
    // COO: moved products first (the fix-up corrects partial 0 and rewrites the receiving outputs of w, which the
    // OTHER workgroups read in phase B: written back to memory before flag A goes up -- the L2s of the XCDs are
    // not coherent with each other inside a launch; nobody has touched those lines of w in this launch yet)
    coo_fixup_body(a.fx);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  }
  if (a.fold_nb) {
    // many partials: chunks by the first fold_nb virtual blocks, as fold_partials_kernel's workgroups
    for (uint32_t base = blockIdx.x * (uint32_t)Q; base < a.fold_nb; base += gridDim.x * (uint32_t)Q) {
      const uint32_t vb = base + q;
      double acc = 0.0;
      if (vb < a.fold_nb) {
        const uint32_t lo = vb * a.fold_chunk, hi = min(a.nparts, lo + a.fold_chunk);
        for (uint32_t i = lo + tq; i < hi; i += 4u * ABFT_BLOCK) {
          double v[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const uint32_t j = i + (uint32_t)k * ABFT_BLOCK;
            v[k] = j < hi ? a.f.partials[j] : 0.0;
          }
          acc += (v[0] + v[1]) + (v[2] + v[3]);
        }
      }
      acc = quarter_sum(acc, s_w);
      if (vb < a.fold_nb && tq == 0) __hip_atomic_store(a.o.partials + vb, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
    }
    if (blockIdx.x * (uint32_t)Q < a.fold_nb && t == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_fetch_add(sync + 8, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (each_a || blockIdx.x == 0) {
    double tot = 0.0, evs = 0.0;
    if (a.fold_nb) {
      if (t == 0) {
        const uint32_t senders = min(gridDim.x, (a.fold_nb + (uint32_t)Q - 1u) / (uint32_t)Q);
        s_last = tail_wait_ge64(sync, 8u, sync[24] + senders, a.timeout_ticks) ? 1u : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      __syncthreads();
      double acc = 0.0;
      for (uint32_t i = tq; i < a.fold_nb; i += ABFT_BLOCK)  // reduce_finish's fold of the chunk sums
        acc += __hip_atomic_load(a.o.partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tot = quarter_sum(acc, s_w);
      if (t == 0 && !s_last) tot = nan;
    } else {
      // fuse_finalize_kernel's fold (1024 threads: fixed order, sixteen independent loads in flight per thread); a
      // smaller workgroup plays 4 / Q of its threads each: the same sixteen wave sums, added in the same order
#pragma unroll
      for (int vt = 0; vt < 4 / Q; vt++) {
        const uint32_t tv = t + (uint32_t)vt * (256u * Q);
        double acc = 0.0;
        for (uint32_t i = tv; i < a.nparts; i += 16u * 1024u) {
          double v[16];
#pragma unroll
          for (int k = 0; k < 16; k++) {
            const uint32_t j = i + (uint32_t)k * 1024u;
            v[k] = j < a.nparts ? a.f.partials[j] : 0.0;
          }
#pragma unroll
          for (int k = 0; k < 16; k += 4) acc += (v[k] + v[k + 1]) + (v[k + 2] + v[k + 3]);
        }
        acc = wave_sum(acc);
        if ((t & 63u) == 63u) s_w[tv >> 6] = acc;
      }
      __syncthreads();
      if (t == 0)
        for (int k = 0; k < 16; k++) tot += s_w[k];
    }
    // (events queued up to the launch's start: the SpMV's -- nothing in this kernel queues any before this point,
    // the COO fix-up aside, whose hand-off form reads the counter behind it)
    if (t == 0) evs = a.fx.on ? (double)__hip_atomic_load(a.f.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (double)nev_a;
    __syncthreads();
    if (a.f.peers.size) peer_allreduce_block(tot, evs, a.f.peers, seq0 + 1ull, false, blockIdx.x == 0);
    if (t == 0) {
      if (blockIdx.x == 0) {  // the pair itself: the caller's, and the next launch's rr / pw
        __hip_atomic_store(a.f.dev_out, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.f.dev_out + 1, evs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!each_a) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(sync + 9, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      s_scal = tot;
    }
  }
  if (!each_a && t == 0) {
    const bool ok = tail_wait_ge64(sync, 9u, gen, a.timeout_ticks);
    const double pw = __hip_atomic_load(a.f.dev_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_scal = ok ? pw : nan;
  }
  __syncthreads();
  // (a launch in which some workgroup gave up waiting leaves the counters short of what the bases say: from then on
  // every launch on this context answers NaN -- loud -- instead of trusting them; sync[30] is never cleared)
  const bool broken = __hip_atomic_load(sync + 30, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;
  const double alpha = broken ? nan : rr / s_scal;  // cg.cpp:102
  __syncthreads();  // (s_scal is written again below)
  TSTAMP(2);

  // ---- B: r -= alpha w; r.r  (calc_r_kernel on a grid of nbv blocks) ----
  if (FAST) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const long i = i0 + (long)k * stride;
      if (myvb < a.nbv && i + 1 < a.n) {
        rv[k].x -= alpha * wv[k].x; rv[k].y -= alpha * wv[k].y;
        *reinterpret_cast<double2 *>(a.r + i) = rv[k];
        acc += rv[k].x * rv[k].x;
        acc += rv[k].y * rv[k].y;
      } else if (myvb < a.nbv && i < a.n) {
        rv[k].x = rv[k].x - alpha * wv[k].x;
        a.r[i] = rv[k].x;
        acc += rv[k].x * rv[k].x;
      }
    }
    acc = quarter_sum(acc, s_w);
    if (myvb < a.nbv && tq == 0) __hip_atomic_store(a.o.partials + myvb, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  } else {
    for (uint32_t base = blockIdx.x * (uint32_t)Q; base < a.nbv; base += gridDim.x * (uint32_t)Q) {
      const uint32_t vb = base + q;
      double acc = 0.0;
      if (vb < a.nbv) {
        for (long i = ((long)vb * ABFT_BLOCK + tq) * VEC; i < a.n; i += stride) {
          if (VEC == 2 && i + 1 < a.n) {
            double2 r2 = *reinterpret_cast<double2 *>(a.r + i);
            const double2 w2 = *reinterpret_cast<const double2 *>(a.w + i);
            r2.x -= alpha * w2.x; r2.y -= alpha * w2.y;
            *reinterpret_cast<double2 *>(a.r + i) = r2;
            acc += r2.x * r2.x;
            acc += r2.y * r2.y;
          } else {
            const double rs = a.r[i] - alpha * a.w[i];
            a.r[i] = rs;
            acc += rs * rs;
          }
        }
      }
      acc = quarter_sum(acc, s_w);
      if (vb < a.nbv && tq == 0) __hip_atomic_store(a.o.partials + vb, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
    }
  }
  if (FAST) {  // phase C's operands, on their way while r.r is being gathered
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const long i = i0 + (long)k * stride;
      pv[k] = xv[k] = make_double2(0.0, 0.0);
      if (myvb < a.nbv && i + 1 < a.n) {
        pv[k] = *reinterpret_cast<const double2 *>(a.p + i);
        xv[k] = *reinterpret_cast<const double2 *>(a.x + i);
      } else if (myvb < a.nbv && i < a.n) {
        pv[k].x = a.p[i];
        xv[k].x = a.x[i];
      }
    }
  }
  TSTAMP(3);
  if (t == 0) {
    uint32_t fold = 0u;
    if (each_b) {
      unsigned long long want[8];
#pragma unroll
      for (uint32_t k = 0; k < 8u; k++) want[k] = sync[16u + k] + (gridDim.x + 7u - k) / 8u;  // workgroups with blockIdx & 7 == k
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (this thread's partial has left; the bases are read)
      (void)__hip_atomic_fetch_add(sync + (blockIdx.x & 7u), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      TSTAMP(4);
      fold = tail_wait_arrivals(sync, want, a.timeout_ticks) ? 1u : 2u;  // everybody folds (2: gave up)
      TSTAMP(5);
    } else {
      // one workgroup folds and publishes (the board lives in host memory: one reader): the last to arrive at ONE counter
      const unsigned long long last = sync[27] + gridDim.x - 1u;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      fold = __hip_atomic_fetch_add(sync + 12, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == last ? 1u : 0u;
    }
    if (fold) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = fold;
  }
  __syncthreads();
  if (s_last) {  // (uniform in the workgroup)
    double acc = 0.0;
    for (uint32_t i = tq; i < a.nbv; i += ABFT_BLOCK)  // fixed order, as reduce_finish
      acc += __hip_atomic_load(a.o.partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc = quarter_sum(acc, s_w);
    double evs = 0.0;
    if (t == 0) {
      evs = (double)__hip_atomic_load(a.o.ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (s_last == 2u) acc = nan;
    }
    // (each_b: workgroup 0 speaks for the rank; else the one workgroup that folds does)
    const bool speaker = !each_b || blockIdx.x == 0;
    if (a.o.peers.size) peer_allreduce_block(acc, evs, a.o.peers, seq0 + 2ull, speaker, speaker);
    if (t == 0) {
      if (speaker) {
        __hip_atomic_store(a.o.dev_out, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.o.dev_out + 1, evs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!each_b) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(sync + 10, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      s_scal = acc;
    }
  }
  __syncthreads();
  if (!each_b && t == 0) {
    const bool ok = tail_wait_ge64(sync, 10u, gen, a.timeout_ticks);
    const double rn = __hip_atomic_load(a.o.dev_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_scal = ok ? rn : nan;
  }
  __syncthreads();
  const double beta = s_scal / rr;  // cg.cpp:109
  TSTAMP(6);

  // ---- C: x += alpha p; p = r + beta p  (calc_px_kernel on the same grid) ----
  if (FAST) {
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const long i = i0 + (long)k * stride;
      if (myvb < a.nbv && i + 1 < a.n) {
        xv[k].x += alpha * pv[k].x; xv[k].y += alpha * pv[k].y;
        pv[k].x = rv[k].x + beta * pv[k].x;
        pv[k].y = rv[k].y + beta * pv[k].y;
        *reinterpret_cast<double2 *>(a.x + i) = xv[k];
        *reinterpret_cast<double2 *>(a.p + i) = pv[k];
      } else if (myvb < a.nbv && i < a.n) {
        a.x[i] = xv[k].x + alpha * pv[k].x;
        a.p[i] = rv[k].x + beta * pv[k].x;
      }
    }
  } else {
    for (uint32_t base = blockIdx.x * (uint32_t)Q; base < a.nbv; base += gridDim.x * (uint32_t)Q) {
      const uint32_t vb = base + q;
      if (vb >= a.nbv) continue;
      for (long i = ((long)vb * ABFT_BLOCK + tq) * VEC; i < a.n; i += stride) {
        if (VEC == 2 && i + 1 < a.n) {
          double2 p2 = *reinterpret_cast<double2 *>(a.p + i);
          double2 x2 = *reinterpret_cast<double2 *>(a.x + i);
          const double2 r2 = *reinterpret_cast<const double2 *>(a.r + i);
          x2.x += alpha * p2.x; x2.y += alpha * p2.y;
          p2.x = r2.x + beta * p2.x;
          p2.y = r2.y + beta * p2.y;
          *reinterpret_cast<double2 *>(a.x + i) = x2;
          *reinterpret_cast<double2 *>(a.p + i) = p2;
        } else {
          const double p1 = a.p[i];
          a.x[i] = a.x[i] + alpha * p1;
          a.p[i] = a.r[i] + beta * p1;
        }
      }
    }
  }
  TSTAMP(7);
  // workgroup 0 leaves the next launch's bases: what this launch's counters stand at once everybody has arrived
  // (everybody HAS read this launch's bases: they are read before the arrival, and phase B is behind us)
  if (blockIdx.x == 0 && t == 0) {
    if (each_b)
      for (uint32_t k = 0; k < 8u; k++) sync[16u + k] += (gridDim.x + 7u - k) / 8u;
    else
      sync[27] += gridDim.x;
    if (a.fold_nb) sync[24] += min(gridDim.x, (a.fold_nb + (uint32_t)Q - 1u) / (uint32_t)Q);
    sync[25] = gen;
  }
}

template <int Q> static int cg_tail_occupancy(bool vec2, bool fast) {
  int n = 0;
  hipError_t e;
  if (fast) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, cg_tail_kernel<2, true, Q>, 256 * Q, 0);
  else if (vec2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, cg_tail_kernel<2, false, Q>, 256 * Q, 0);
  else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, cg_tail_kernel<1, false, Q>, 256 * Q, 0);
  if (e != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}
int cg_tail_blocks_per_cu(bool vec2, bool fast, int q) {
  return q == 4 ? cg_tail_occupancy<4>(vec2, fast) : q == 2 ? cg_tail_occupancy<2>(vec2, fast) : cg_tail_occupancy<1>(vec2, fast);
}

template <int Q> static void launch_cg_tail_q(const TailArgs &a, bool vec2, bool fast, uint32_t grid, hipStream_t s) {
  if (fast) hipLaunchKernelGGL((cg_tail_kernel<2, true, Q>), dim3(grid), dim3(256 * Q), 0, s, a);
  else if (vec2) hipLaunchKernelGGL((cg_tail_kernel<2, false, Q>), dim3(grid), dim3(256 * Q), 0, s, a);
  else hipLaunchKernelGGL((cg_tail_kernel<1, false, Q>), dim3(grid), dim3(256 * Q), 0, s, a);
}
hipError_t launch_cg_tail(const TailArgs &a, bool vec2, bool fast, int q, uint32_t grid, hipStream_t s) {
  if (q == 4) launch_cg_tail_q<4>(a, vec2, fast, grid, s);
  else if (q == 2) launch_cg_tail_q<2>(a, vec2, fast, grid, s);
  else launch_cg_tail_q<1>(a, vec2, fast, grid, s);
  return hipGetLastError();
}

// {value, count} in device memory (e.g. what a collective left there) -> the pinned host
// slot, published like a reduction's result so the host can poll for it
__global__ void publish_pair_kernel(const double *pair, HostSlot *host, uint32_t seq) {
  const double v = __hip_atomic_load(pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double c = __hip_atomic_load(pair + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&host->value, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host->evcount, c > 0.0 ? (c < 4.0e9 ? (uint32_t)c : 0xffffffffu) : 0u, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&host->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_publish_pair(const double *pair, HostSlot *host, uint32_t seq, hipStream_t s) {
  hipLaunchKernelGGL(publish_pair_kernel, dim3(1), dim3(1), 0, s, pair, host, seq);
  return hipGetLastError();
}

// ---------------------------------------------- all-reduce of a pair over a peer board --
//
// The two scalar reductions of a CG iteration across the processes of one node (one per
// GPU), without a collective library: 16 bytes per rank.  The board is a few KB of pinned
// host memory that every process of the job has mapped and registered (POSIX shared memory),
// two rows (the parity of the reduction's sequence number) of one 32-byte slot per rank.  A
// rank stores {value, events} and then the sequence number into ITS slot with system-scope
// stores -- posted writes of one device arrive in order -- and the lanes of one wave poll the
// slots of all ranks until they carry this sequence number; lane 0 adds them in rank order,
// so every rank forms the same bits.  Two rows are enough: a rank can start reduction k + 1
// (other row) before a slow peer has read row k, but not k + 2, which needs that peer's
// k + 1.  One kernel node: capturable, nothing to set up at first use, and the latency is two
// PCIe crossings instead of a collective's launch and protocol.  Every wait is bounded; a
// rank that gives up leaves NaN and raises its flag on the board.
__global__ __launch_bounds__(64) void peer_allreduce_kernel(double *pair, PeerArgs P) {
  double v0 = 0.0, v1 = 0.0;
  if (threadIdx.x == 0) {
    v0 = pair[0];
    v1 = pair[1];
  }
  peer_allreduce_block(v0, v1, P);
  if (threadIdx.x == 0) {
    pair[0] = v0;
    pair[1] = v1;
  }
}

hipError_t launch_peer_allreduce(double *pair, const PeerArgs &P, hipStream_t s) {
  hipLaunchKernelGGL(peer_allreduce_kernel, dim3(1), dim3(64), 0, s, pair, P);
  return hipGetLastError();
}

// ------------------------------------------ window exchange over shared host memory --
//
// The halo of a banded matrix in front of a row-partitioned SpMV (a few KB to a few hundred
// KB per neighbour) between the processes of one node, in ONE kernel: every rank copies the
// windows its peers read out of its slot of the gathered vector into its outbox in shared
// host memory, publishes the sequence number, waits for the ranks it reads from and copies
// their windows into its own gathered vector.  Outboxes are doubled by the parity of the
// sequence number; before a rank overwrites an outbox it waits until its readers have
// finished with the exchange two back (`done`), so the protocol does not lean on whatever
// else synchronises the ranks in between.  Capturable, bounded waits, NaN + flag on give-up.
__device__ __forceinline__ bool peer_wait_ge(const unsigned long long *word, unsigned long long want,
                                             unsigned long long timeout_ticks) {
  const unsigned long long t0 = (unsigned long long)wall_clock64();
  while (sys_load_b64(word) < want) {
    if ((unsigned long long)wall_clock64() - t0 > timeout_ticks) return false;
    __builtin_amdgcn_s_sleep(4);
  }
  return true;
}

// xor of `x` over the block into s_x[0..1] (low, high half): inside each wave by lane exchange, then
// one LDS atomic pair per wave (1024 threads on two LDS words took 3.5 us, measured)
__device__ __forceinline__ void block_xor_into(uint32_t *s_x, unsigned long long x) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    lo ^= (uint32_t)__shfl_xor((int)lo, m);
    hi ^= (uint32_t)__shfl_xor((int)hi, m);
  }
  if ((threadIdx.x & 63u) == 0u) {
    atomicXor(&s_x[0], lo);
    atomicXor(&s_x[1], hi);
  }
}

__global__ __launch_bounds__(1024) void peer_exchange_kernel(const PeerExchange *Xp, double *__restrict__ full) {
  __shared__ uint32_t s_bad, s_retry;
  __shared__ uint32_t s_x[2];  // xor of the 64-bit words of the window in hand, as two halves
  const PeerExchange &X = *Xp;
  const uint32_t t = threadIdx.x;
  const unsigned long long seq = *X.counter + 1ull;
  const unsigned long long q = seq & 1ull;
  const unsigned long long salt = seq * 0x9E3779B97F4A7C15ull;
  // Two transports, one protocol.  Shared host memory (X.regions == NULL): one region all ranks map; a rank
  // copies its windows into ITS outbox there and the readers pull them.  Device memory (round 3): every rank
  // has a region of the same layout in its own GPU's memory, the peers' regions mapped over IPC
  // (X.regions[r]); a rank PUSHES each window into the reader's region -- into the box that stands for
  // (this sender, parity) there -- and its `ready` / `done` words into the peers' headers; every wait
  // and every read is then on the rank's own memory.
  unsigned char *const local = X.regions ? X.regions[X.rank] : X.shared;
  unsigned long long *ready = reinterpret_cast<unsigned long long *>(local);
  unsigned long long *done = ready + ABFT_PEER_MAX_RANKS;
  uint32_t *fail = reinterpret_cast<uint32_t *>(done + ABFT_PEER_MAX_RANKS);
  if (t == 0) s_bad = 0u;
#ifdef ABFT_DBG_STAMPS  // timing build: wall-clock stamps (10 ns) of the phases, left in the header's spare half
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define XSTAMP(k) st[k] = (unsigned long long)wall_clock64()
#else
#define XSTAMP(k)
#endif
  XSTAMP(0);
  __syncthreads();
  // The readers of the outbox about to be overwritten are through with exchange seq - 2.  For a
  // reader this rank also reads from that is known already: it published exchange seq - 1, which
  // the last exchange waited for, and its stream runs its exchanges one after the other.  Only a
  // reader this rank takes nothing from (pad != 0) is asked, which costs a trip across the link.
  if (t < (uint32_t)X.nout && X.out[t].pad && seq > 2ull && !peer_wait_ge(done + X.out[t].peer, seq - 2ull, X.timeout_ticks))
    atomicOr(&s_bad, 1u);
  __syncthreads();
  XSTAMP(1);
  for (int k = 0; k < X.nout; k++) {
    const PeerPiece pc = X.out[k];
    unsigned char *mybox = (X.regions ? X.regions[pc.peer] : X.shared) + ABFT_PEER_XHDR_BYTES +
                           ((size_t)X.rank * 2u + q) * X.box_bytes;
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(mybox + pc.box_off);
    const double *src = full + pc.vec_off;
    if (t < 2u) s_x[t] = 0u;
    __syncthreads();
    unsigned long long x = 0ull;
    const uint32_t npair = (pc.box_off & 15ull) == 0ull ? pc.count / 2u : 0u;
    for (uint32_t j = t; j < npair; j += 1024u) {
      const unsigned long long w0 = (unsigned long long)__double_as_longlong(src[2u * j]);
      const unsigned long long w1 = (unsigned long long)__double_as_longlong(src[2u * j + 1u]);
      x ^= w0 ^ w1;
      sys_store_b128(reinterpret_cast<u64x2 *>(dst + 2u * j), u64x2{w0, w1});
    }
    for (uint32_t i = 2u * npair + t; i < pc.count; i += 1024u) {
      const unsigned long long w = (unsigned long long)__double_as_longlong(src[i]);
      x ^= w;
      sys_store_b64(dst + i, w);
    }
    block_xor_into(s_x, x);
    __syncthreads();
    // behind the window: a word that ties its contents to this exchange (see the reader)
    if (t == 0) sys_store_b64(dst + pc.count, ((unsigned long long)s_x[1] << 32 | s_x[0]) ^ salt);
    __syncthreads();
  }
  XSTAMP(2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every thread: its stores have been taken
  __syncthreads();
  XSTAMP(3);
  if (X.regions) {  // into every reader's header (a reader with several windows is told several times: the same word)
    if (t < (uint32_t)X.nout)
      sys_store_b64(reinterpret_cast<unsigned long long *>(X.regions[X.out[t].peer]) + X.rank, seq);
  } else if (t == 0) {
    sys_store_b64(ready + X.rank, seq);
  }
  if (t < (uint32_t)X.nin && !peer_wait_ge(ready + X.in[t].peer, seq, X.timeout_ticks)) atomicOr(&s_bad, 1u);
  __syncthreads();
  XSTAMP(4);
  for (int k = 0; k < X.nin && !s_bad; k++) {
    const PeerPiece pc = X.in[k];
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(
        local + ABFT_PEER_XHDR_BYTES + ((size_t)pc.peer * 2u + q) * X.box_bytes + pc.box_off);
    double *dst = full + pc.vec_off;
    // The sender stored the window, waited for those stores, then stored the sequence number this
    // rank has now seen.  The check word makes a window that is not (yet) what its sender wrote for
    // THIS exchange a re-read instead of a silently stale halo, whatever reorders stores on the way.
    const unsigned long long t0 = (unsigned long long)wall_clock64();
    const uint32_t npair = (pc.box_off & 15ull) == 0ull ? pc.count / 2u : 0u;
    for (;;) {
      if (t < 2u) s_x[t] = 0u;
      if (t == 0) s_retry = 0u;
      __syncthreads();
      unsigned long long x = 0ull, want = 0ull;
      if (t == 1023u) want = sys_load_b64(src + pc.count);
      for (uint32_t j0 = t; j0 < npair; j0 += 4096u) {  // four 16-byte loads across the link in flight per thread
        const u64x2 *base = reinterpret_cast<const u64x2 *>(src);
        const uint32_t j1 = j0 + 1024u, j2 = j0 + 2048u, j3 = j0 + 3072u;
        u64x2 w0, w1, w2, w3;
        sys_load4_b128(base + j0, base + (j1 < npair ? j1 : j0), base + (j2 < npair ? j2 : j0), base + (j3 < npair ? j3 : j0),
                       w0, w1, w2, w3);
        x ^= w0.x ^ w0.y;
        dst[2u * j0] = __longlong_as_double((long long)w0.x);
        dst[2u * j0 + 1u] = __longlong_as_double((long long)w0.y);
        if (j1 < npair) {
          x ^= w1.x ^ w1.y;
          dst[2u * j1] = __longlong_as_double((long long)w1.x);
          dst[2u * j1 + 1u] = __longlong_as_double((long long)w1.y);
        }
        if (j2 < npair) {
          x ^= w2.x ^ w2.y;
          dst[2u * j2] = __longlong_as_double((long long)w2.x);
          dst[2u * j2 + 1u] = __longlong_as_double((long long)w2.y);
        }
        if (j3 < npair) {
          x ^= w3.x ^ w3.y;
          dst[2u * j3] = __longlong_as_double((long long)w3.x);
          dst[2u * j3 + 1u] = __longlong_as_double((long long)w3.y);
        }
      }
      for (uint32_t i = 2u * npair + t; i < pc.count; i += 1024u) {
        const unsigned long long w = sys_load_b64(src + i);
        x ^= w;
        dst[i] = __longlong_as_double((long long)w);
      }
      x ^= want;  // (thread 1023 folds the sender's word in: the total must come out as the salt)
      block_xor_into(s_x, x);
      __syncthreads();
      if (t == 0 && ((unsigned long long)s_x[1] << 32 | s_x[0]) != salt) {
        if ((unsigned long long)wall_clock64() - t0 > X.timeout_ticks) s_bad = 1u;
        else s_retry = 1u;
      }
      __syncthreads();
      if (!s_retry) break;
      __builtin_amdgcn_s_sleep(16);
    }
  }
  __syncthreads();
  XSTAMP(5);
#ifdef ABFT_DBG_STAMPS
  if (t == 0)
    for (int k = 0; k < 6; k++) sys_store_b64(ready + 256 + X.rank * 8 + k, st[k]);
#endif
  if (t == 0) {
    if (s_bad) {
      if (X.nin > 0) full[X.in[0].vec_off] = __longlong_as_double(0x7ff8000000000000ll);
      __hip_atomic_store(fail + X.rank, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!X.regions) sys_store_b64(done + X.rank, seq);  // (every load of this block has returned: the barrier above)
    *X.counter = seq;
  }
  // device memory: "through with exchange seq" goes into the header of every rank this one reads from
  if (X.regions && t < (uint32_t)X.nin)
    sys_store_b64(reinterpret_cast<unsigned long long *>(X.regions[X.in[t].peer]) + ABFT_PEER_MAX_RANKS + X.rank, seq);
}

hipError_t launch_peer_exchange(const PeerExchange *X, double *full, hipStream_t s) {
  hipLaunchKernelGGL(peer_exchange_kernel, dim3(1), dim3(1024), 0, s, X, full);
  return hipGetLastError();
}

// copy_vector (reference CSR/CPUContext.cpp:76-80: memcpy of dst->N doubles), as an
// ordinary kernel on the context's stream (capturable; no runtime copy path involved)
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void copy_kernel(double *__restrict__ dst, const double *__restrict__ src,
                                                          int n) {
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n)
      *reinterpret_cast<double2 *>(dst + i) = *reinterpret_cast<const double2 *>(src + i);
    else
      dst[i] = src[i];
  }
}

hipError_t launch_copy(double *dst, const double *src, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  long nb = ((long)n + ABFT_BLOCK * 4 - 1) / (ABFT_BLOCK * 4);
  if (nb > 4096) nb = 4096;
  ABFT_VEC_DISPATCH(copy_kernel, (), aligned16(dst, src), (unsigned)nb, dst, src, n);
  return hipGetLastError();
}

// ------------------------------------------------------------ bandwidth probe --

// (four 16-byte non-temporal loads in flight per thread, then four non-temporal stores: the plain
// one-load-one-store grid-stride loop of rounds 1-3 reached 4.9 TB/s where the read probe reaches 6.4)
__global__ __launch_bounds__(ABFT_BLOCK) void stream_copy_kernel(double2 *__restrict__ dst,
                                                                 const double2 *__restrict__ src, size_t n2) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v2d *s = reinterpret_cast<const v2d *>(src);
  v2d *d = reinterpret_cast<v2d *>(dst);
  const size_t stride = (size_t)gridDim.x * ABFT_BLOCK * 4;
  for (size_t base = (size_t)blockIdx.x * ABFT_BLOCK * 4 + threadIdx.x; base < n2; base += stride) {
    v2d v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const size_t i = base + (size_t)k * ABFT_BLOCK;
      v[k] = i < n2 ? __builtin_nontemporal_load(s + i) : v2d{0.0, 0.0};
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const size_t i = base + (size_t)k * ABFT_BLOCK;
      if (i < n2) __builtin_nontemporal_store(v[k], d + i);
    }
  }
}

__global__ __launch_bounds__(ABFT_BLOCK) void stream_read_kernel(const double2 *__restrict__ src, size_t n2,
                                                                 double *sink) {
  const size_t stride = (size_t)gridDim.x * ABFT_BLOCK;
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * ABFT_BLOCK + threadIdx.x; i < n2; i += stride) {
    const double2 v = src[i];
    acc += v.x + v.y;
  }
  if (acc == 1.2345e-300) *sink = acc;  // keeps the loads alive, never true in practice
}

hipError_t launch_stream_copy(double *dst, const double *src, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(stream_copy_kernel, dim3(256 * 8), dim3(ABFT_BLOCK), 0, s, (double2 *)dst,
                     (const double2 *)src, n / 2);
  return hipGetLastError();
}
hipError_t launch_stream_read(const double *src, size_t n, double *sink, hipStream_t s) {
  hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 8), dim3(ABFT_BLOCK), 0, s, (const double2 *)src, n / 2,
                     sink);
  return hipGetLastError();
}

// ----------------------------------------------------------- matrix digests --
// D(segment) = sum w[i] (2 i + 1) mod 2^64 over every segment of a matrix in ONE launch (matrix_digest.h, DESIGN.md
// section 5u).  A plain read stream: every workgroup walks the table; per segment it takes its grid-stride share of
// the 16-byte groups, four loads in flight per lane, one 32 x 32 -> 64 multiply-add per word into a 64-bit register
// pair, folds the lanes over DPP and the four waves through LDS, and thread 0 adds the workgroup's share onto the
// segment's accumulator with one 64-bit integer atomic.  Integer addition commutes, so the accumulator holds the same
// bits whatever the order.  A workgroup with no share of a segment (most of them, on the small tables) skips it
// without a barrier or an atomic: the test is uniform over the workgroup.  The bytes behind the last full group
// (0..15, the last word zero-extended) are workgroup 0's, read byte by byte: nothing is loaded past the segment.
typedef __attribute__((address_space(1))) u32x4 GlobalQuad;
__device__ __forceinline__ unsigned long long digest_quad(unsigned long long acc, u32x4 v, uint32_t q) {
  acc = digest_term(acc, v.x, 4u * q);
  acc = digest_term(acc, v.y, 4u * q + 1u);
  acc = digest_term(acc, v.z, 4u * q + 2u);
  return digest_term(acc, v.w, 4u * q + 3u);
}

__global__ __launch_bounds__(ABFT_BLOCK) void matrix_digest_kernel(const DigestSeg *__restrict__ table, uint32_t nseg,
                                                                   unsigned long long *__restrict__ acc) {
  __shared__ unsigned long long wave_sum[ABFT_BLOCK / 64];
  constexpr uint32_t PER_BLOCK = 4u * ABFT_BLOCK;  // groups a workgroup takes per step
  const uint32_t first = blockIdx.x * PER_BLOCK, step = gridDim.x * PER_BLOCK;
  for (uint32_t s = 0; s < nseg; s++) {
    const DigestSeg seg = table[s];
    const bool tail_here = blockIdx.x == 0u && seg.tail != 0u;
    if (first >= seg.quads && !tail_here) continue;  // uniform over the workgroup
    // (the table hands the pointer over as a generic one: say that it is device memory, for global loads)
    const GlobalQuad *src = (const GlobalQuad *)seg.base;
    unsigned long long sum = 0ull;
    // whole steps, nothing predicated (quads <= 2^29 and step <= 2^21: base never wraps) ...
    uint32_t base = first + threadIdx.x;
    for (; base + 3u * ABFT_BLOCK < seg.quads; base += step) {
      u32x4 v[4];
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) v[k] = STREAM_LOAD(src + base + k * ABFT_BLOCK);
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) sum = digest_quad(sum, v[k], base + k * ABFT_BLOCK);
    }
    // ... and the one step that is cut short (base + step lies past the end: base + 3 * ABFT_BLOCK did already)
    if (base < seg.quads) {
      u32x4 v[4];
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t q = base + k * ABFT_BLOCK;
        v[k] = q < seg.quads ? STREAM_LOAD(src + q) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) sum = digest_quad(sum, v[k], base + k * ABFT_BLOCK);  // (a zero word adds nothing)
    }
    if (tail_here && threadIdx.x < (seg.tail + 3u) / 4u) {
      const unsigned char *p = static_cast<const unsigned char *>(seg.base) + (size_t)seg.quads * 16u + 4u * threadIdx.x;
      const uint32_t left = seg.tail - 4u * threadIdx.x;
      sum = digest_term(sum, digest_tail_word(p, left < 4u ? left : 4u), 4u * seg.quads + threadIdx.x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    __syncthreads();  // the previous segment's sums have been read
    if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
      unsigned long long total = 0ull;
#pragma unroll
      for (int w = 0; w < ABFT_BLOCK / 64; w++) total += wave_sum[w];
      atomicAdd(acc + s, total);
    }
  }
}

// One workgroup, in stream order behind matrix_digest_kernel: that order is all the ordering there is.
__global__ __launch_bounds__(64) void matrix_digest_finish_kernel(const DigestSeg *__restrict__ table, uint32_t nseg,
                                                                  unsigned long long *__restrict__ acc,
                                                                  const unsigned long long *__restrict__ ref,
                                                                  unsigned long long *__restrict__ pairs, EventRing ev,
                                                                  uint32_t fmt) {
  const uint32_t s = threadIdx.x;
  if (s >= nseg) return;
  const unsigned long long now = acc[s], armed = ref[s];
  pairs[2u * s] = now;
  pairs[2u * s + 1u] = armed;
  if (now != armed) push_event(ev, ABFT_EV_MATRIX_DIGEST, table[s].kind, 0u, fmt);
  acc[s] = 0ull;
}

hipError_t launch_matrix_digest(const DigestSeg *table, uint32_t nseg, unsigned long long *acc, uint32_t grid, hipStream_t s) {
  hipLaunchKernelGGL(matrix_digest_kernel, dim3(grid), dim3(ABFT_BLOCK), 0, s, table, nseg, acc);
  return hipGetLastError();
}
hipError_t launch_matrix_digest_finish(const DigestSeg *table, uint32_t nseg, unsigned long long *acc,
                                       const unsigned long long *ref, unsigned long long *pairs, EventRing ev, uint32_t fmt,
                                       hipStream_t s) {
  hipLaunchKernelGGL(matrix_digest_finish_kernel, dim3(1), dim3(64), 0, s, table, nseg, acc, ref, pairs, ev, fmt);
  return hipGetLastError();
}

// ------------------------------------------------------- protected vectors --
// The vector kernels of the abft_hip_*_vecc entries (the code: ecc_device.h).
// Each walks its vectors exactly as its plain counterpart does -- same grid, stride, VEC by alignment,
// block_sum and last-block fold --, decodes every word it loads, computes in full fp64 with separate
// multiply and add, and encodes every word it stores; sums are over the values as stored.
//
// The hot loops hold no call (section 4, "Round 4, late"): a step with a word that fails its check is
// only NOTED -- nothing of it is stored or summed -- and behind the loop a thread with a noted step walks
// its chain once more.  There a step that is clean has been carried out (its outputs are codewords
// again, its read-only inputs always were) and adds the stored values it left; a step that still fails is
// the noted one: vecc_cold repairs its words in registers (an input that is only read is not written
// back), the step is carried out and adds what it stores.  Same operands and the same order of adds as an
// undamaged call, so every vector and the sum have the undamaged call's bits.
//
// That discipline is written ONCE, in vecc_walk.h: vecc_walk is the two walks, an operation
// (VeccDot, VeccCalcXr, ...) states its arithmetic and its sums once, and a kernel here is vecc_grid_walk with its
// operation, the operands in the order its entry reports them, and then its reduction.  vecc_walk.h includes nothing
// of HIP: tests/test_vecc_walk_host.py runs the same text on a CPU.  Two walks keep their hand-written form
// (calc_px_vecc_walk, precond_start_vecc_walk): section 5p says why.

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void vector_encode_kernel(double *__restrict__ v, int n) {
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  for (long i = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      double2 t = *reinterpret_cast<double2 *>(v + i);
      t.x = vecc_double(vecc_encode(t.x));
      t.y = vecc_double(vecc_encode(t.y));
      *reinterpret_cast<double2 *>(v + i) = t;
    } else {
      v[i] = vecc_double(vecc_encode(v[i]));
    }
  }
}

// A thread's chain in the grid of the vector kernels under vecc_walk (vecc_walk.h): the hot loop, and behind it the
// second walk of a thread with a noted step
template <int VEC, class OP, class COLD>
__device__ __forceinline__ void vecc_grid_walk(const OP &op, const VeccOperands<OP> &o, int n, COLD &cold, double *acc) {
  vecc_walk<VEC>(op, o, n, ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC, (long)gridDim.x * ABFT_BLOCK * VEC, cold,
                 acc);
}

// the scrub's cold decode: vecc_cold, counted
struct VeccColdScrub {
  EventRing ev;
  uint32_t fixed, lost;
  __device__ __forceinline__ VeccWord operator()(uint64_t word, uint32_t index, uint32_t operand) {
    const VeccWord o = vecc_cold(word, index, operand, ev);
    if (o.rc > 0) fixed++;
    else lost++;
    return o;
  }
};

// counts[0] += words repaired (and written back), counts[1] += words with two flipped bits (left as they are)
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void vector_scrub_kernel(double *__restrict__ v, int n, uint32_t *counts,
                                                                  EventRing ev) {
  VeccColdScrub cold{ev, 0u, 0u};
  vecc_grid_walk<VEC>(VeccScrub{}, VeccOperands<VeccScrub>{{v}, {0u}}, n, cold, nullptr);
  if (cold.fixed) atomicAdd(counts, cold.fixed);
  if (cold.lost) atomicAdd(counts + 1, cold.lost);
}

// dot on protected vectors: operands 0 (a) and 1 (b), neither written back
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void dot_vecc_kernel(const double *__restrict__ a,
                                                              const double *__restrict__ b, int n,
                                                              ReduceOut out, EventRing ev) {
  __shared__ double s_w[4];
  double acc = 0.0;
  VeccColdDev cold{ev};
  vecc_grid_walk<VEC>(VeccDot{}, VeccOperands<VeccDot>{{const_cast<double *>(a), const_cast<double *>(b)}, {0u, 1u}}, n,
                      cold, &acc);
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// calc_xr on protected vectors: x += alpha p; r -= alpha w (operands 0..3); r.r over the r it stores
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_xr_vecc_kernel(double *__restrict__ x, double *__restrict__ r,
                                                                  const double *__restrict__ p,
                                                                  const double *__restrict__ w, double alpha, int n,
                                                                  ReduceOut out, EventRing ev) {
  __shared__ double s_w[4];
  double acc = 0.0;
  VeccColdDev cold{ev};
  vecc_grid_walk<VEC>(VeccCalcXr{alpha},
                      VeccOperands<VeccCalcXr>{{x, r, const_cast<double *>(p), const_cast<double *>(w)}, {0u, 1u, 2u, 3u}},
                      n, cold, &acc);
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// calc_p on protected vectors: p = r + beta p (operands 0: p, 1: r); p is left repaired, r not written back
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_p_vecc_kernel(double *__restrict__ p, const double *__restrict__ r,
                                                                 double beta, int n, EventRing ev) {
  VeccColdDev cold{ev};
  vecc_grid_walk<VEC>(VeccCalcP{beta}, VeccOperands<VeccCalcP>{{p, const_cast<double *>(r)}, {0u, 1u}}, n, cold, nullptr);
}

hipError_t launch_vector_encode(double *v, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(vector_encode_kernel, (), aligned16(v), nb, v, n);
  return hipGetLastError();
}

hipError_t launch_vector_scrub(double *v, int n, uint32_t *counts, EventRing ev, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(vector_scrub_kernel, (), aligned16(v), nb, v, n, counts, ev);
  return hipGetLastError();
}

hipError_t launch_dot_vecc(const double *a, const double *b, int n, const ReduceOut &out, EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(dot_vecc_kernel, (), aligned16(a, b), nb, a, b, n, out, ev);
  return hipGetLastError();
}

hipError_t launch_calc_xr_vecc(double *x, double *r, const double *p, const double *w, double alpha, int n,
                               const ReduceOut &out, EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_xr_vecc_kernel, (), aligned16(x, r, p, w), nb, x, r, p, w, alpha, n, out, ev);
  return hipGetLastError();
}

hipError_t launch_calc_p_vecc(double *p, const double *r, double beta, int n, EventRing ev, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_p_vecc_kernel, (), aligned16(p, r), nb, p, r, beta, n, ev);
  return hipGetLastError();
}

// ---- the two-kernel tail on protected vectors (abft_hip_calc_r_vecc, abft_hip_calc_px_vecc) and the guarded
// iteration built on it (abft_hip_cg_vecc_iteration_until_dev) ----
// calc_xr_vecc_kernel cut where calc_r_kernel / calc_px_kernel cut calc_xr_kernel: the r half alone, and the x half
// moved into calc_p's pass over p, so that p is read once per iteration.  Same discipline as above -- no call in
// the hot loops, a step with a suspect word only noted, the chain walked once more behind the loop -- and per element
// the same operands and roundings, per thread the same order of adds: with the walk chosen alike (VEC, by the
// alignment of the operands) x, r and r.r have calc_xr_vecc's bits and p has calc_p_vecc's.
// ONE body per pair (section 5i): the host-scalar kernel and the guarded one call the same walk -- the r half
// vecc_walk with VeccCalcR<false>, the x / p half written out (section 5p).  op_*: the ordinal
// a repaired word of that vector is reported under -- the host-scalar entries count their own arguments, the guarded
// entry counts vec, x, r, p, w as 0..4.

// r <- enc(dec(r) - alpha dec(w)) over the grid -> this thread's serial sum of the stored r's squares; w is not written back
template <int VEC>
__device__ __forceinline__ double calc_r_vecc_walk(double *__restrict__ r, const double *__restrict__ w, double alpha,
                                                   int n, uint32_t op_r, uint32_t op_w, EventRing ev) {
  double acc = 0.0;
  VeccColdDev cold{ev};
  vecc_grid_walk<VEC>(VeccCalcR<false>{alpha}, VeccOperands<VeccCalcR<false>>{{r, const_cast<double *>(w)}, {op_r, op_w}},
                      n, cold, &acc);
  return acc;
}

// (this walk keeps its hand-written form: under vecc_walk its VEC == 2 instances took one VGPR more)
// x <- enc(dec(x) + alpha dec(p)) and p <- enc(dec(r) + beta dec(p)) in one pass over p, both from the old p;
// r is not written back
template <int VEC>
__device__ __forceinline__ void calc_px_vecc_walk(double *__restrict__ x, double *__restrict__ p,
                                                  const double *__restrict__ r, double alpha, double beta, int n,
                                                  uint32_t op_x, uint32_t op_p, uint32_t op_r, EventRing ev) {
  uint32_t bad = 0u;
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  const long first = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC;
  for (long i = first; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      const double2 pv = *reinterpret_cast<const double2 *>(p + i);
      const double2 xv = *reinterpret_cast<const double2 *>(x + i);
      const double2 rv = *reinterpret_cast<const double2 *>(r + i);
      const uint64_t p0 = vecc_bits(pv.x), p1 = vecc_bits(pv.y), x0 = vecc_bits(xv.x), x1 = vecc_bits(xv.y);
      const uint64_t r0 = vecc_bits(rv.x), r1 = vecc_bits(rv.y);
      const uint32_t sus = (vecc_suspect(p0) | vecc_suspect(p1)) | (vecc_suspect(x0) | vecc_suspect(x1)) |
                           (vecc_suspect(r0) | vecc_suspect(r1));
      bad |= sus;
      if (!sus) {
        const uint64_t xs0 = vecc_encode(vecc_value(x0) + alpha * vecc_value(p0));
        const uint64_t xs1 = vecc_encode(vecc_value(x1) + alpha * vecc_value(p1));
        const uint64_t q0 = vecc_encode(vecc_value(r0) + beta * vecc_value(p0));
        const uint64_t q1 = vecc_encode(vecc_value(r1) + beta * vecc_value(p1));
        *reinterpret_cast<double2 *>(x + i) = make_double2(vecc_double(xs0), vecc_double(xs1));
        *reinterpret_cast<double2 *>(p + i) = make_double2(vecc_double(q0), vecc_double(q1));
      }
    } else {
      const uint64_t p0 = vecc_bits(p[i]), x0 = vecc_bits(x[i]), r0 = vecc_bits(r[i]);
      const uint32_t sus = vecc_suspect(p0) | vecc_suspect(x0) | vecc_suspect(r0);
      bad |= sus;
      if (!sus) {
        x[i] = vecc_double(vecc_encode(vecc_value(x0) + alpha * vecc_value(p0)));
        p[i] = vecc_double(vecc_encode(vecc_value(r0) + beta * vecc_value(p0)));
      }
    }
  }
  if (__builtin_expect(bad != 0u, 0)) {
    for (long i = first; i < n; i += stride) {
      const int m = (VEC == 2 && i + 1 < n) ? 2 : 1;
      uint32_t sus = 0u;
      for (int k = 0; k < m; k++)
        sus |= vecc_suspect(vecc_bits(p[i + k])) | vecc_suspect(vecc_bits(x[i + k])) | vecc_suspect(vecc_bits(r[i + k]));
      if (!sus) continue;  // carried out above
      for (int k = 0; k < m; k++) {
        const uint32_t j = (uint32_t)(i + k);
        const double xo = vecc_decode_cold_ok(x + i + k, j, op_x, ev);
        const double po = vecc_decode_cold_ok(p + i + k, j, op_p, ev);
        const double ro = vecc_decode_cold_ok(r + i + k, j, op_r, ev);
        x[i + k] = vecc_double(vecc_encode(xo + alpha * po));
        p[i + k] = vecc_double(vecc_encode(ro + beta * po));
      }
    }
  }
}

// calc_r on protected vectors: r -= alpha w (operands 0: r, 1: w); r.r over the r it stores
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_vecc_kernel(double *__restrict__ r, const double *__restrict__ w,
                                                                 double alpha, int n, ReduceOut out, EventRing ev) {
  __shared__ double s_w[4];
  double acc = calc_r_vecc_walk<VEC>(r, w, alpha, n, 0u, 1u, ev);
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

// calc_px on protected vectors: x += alpha p; p = r + beta p (operands 0: x, 1: p, 2: r)
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_vecc_kernel(double *__restrict__ x, double *__restrict__ p,
                                                                  const double *__restrict__ r, double alpha,
                                                                  double beta, int n, EventRing ev) {
  calc_px_vecc_walk<VEC>(x, p, r, alpha, beta, n, 0u, 1u, 2u, ev);
}

// The guarded forms: calc_r_until_kernel and calc_px_until_kernel with the protected walks.  Operands as the guarded
// entry counts them: x 1, r 2, p 3, w 4 (0 is the SpMV's gathered vector).  A frozen launch touches no vector: it
// repairs nothing and reports nothing.
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_vecc_until_kernel(double *__restrict__ r,
                                                                       const double *__restrict__ w, const double *rr,
                                                                       const double *pw, double threshold,
                                                                       double *alpha_out, int n, ReduceOut out,
                                                                       EventRing ev) {
  __shared__ double s_w[4];
  double alpha;
  if (!guard_r_head<GuardPair>(rr, pw, threshold, alpha_out, out, &alpha)) return;
  double acc = calc_r_vecc_walk<VEC>(r, w, alpha, n, 2u, 4u, ev);
  acc = block_sum(acc, s_w);
  reduce_finish(acc, out, s_w);
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_vecc_until_kernel(double *__restrict__ x, double *__restrict__ p,
                                                                        const double *__restrict__ r, const double *rr,
                                                                        const double *rr_new, double threshold,
                                                                        const double *alpha_ptr, int n, EventRing ev) {
  if (!GuardPair::live(rr, threshold)) return;
  const double beta = GuardPair::beta(rr, rr_new);
  const double alpha = *alpha_ptr;
  calc_px_vecc_walk<VEC>(x, p, r, alpha, beta, n, 1u, 3u, 2u, ev);
}

// (each half chooses its walk over its own operands, in the host-scalar and in the guarded form alike: a live guarded
// iteration has the bits of the two host-scalar calls whatever the alignment of the vectors it does not touch)
hipError_t launch_calc_r_vecc(double *r, const double *w, double alpha, int n, const ReduceOut &out, EventRing ev,
                              hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_r_vecc_kernel, (), aligned16(r, w), nb, r, w, alpha, n, out, ev);
  return hipGetLastError();
}

hipError_t launch_calc_px_vecc(double *x, double *p, const double *r, double alpha, double beta, int n, EventRing ev,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_px_vecc_kernel, (), aligned16(x, p, r), nb, x, p, r, alpha, beta, n, ev);
  return hipGetLastError();
}

hipError_t launch_calc_r_vecc_until(double *r, const double *w, const double *rr, const double *pw, double threshold,
                                    double *alpha_out, int n, const ReduceOut &out, EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_r_vecc_until_kernel, (), aligned16(r, w), nb, r, w, rr, pw, threshold, alpha_out, n, out, ev);
  return hipGetLastError();
}

hipError_t launch_calc_px_vecc_until(double *x, double *p, const double *r, const double *rr, const double *rr_new,
                                     double threshold, const double *alpha_ptr, int n, EventRing ev, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_px_vecc_until_kernel, (), aligned16(x, p, r), nb, x, p, r, rr, rr_new, threshold, alpha_ptr, n,
                    ev);
  return hipGetLastError();
}

// ---- protected block vectors (abft_hip_dot_block_vecc, abft_hip_calc_r_block_vecc, abft_hip_calc_px_block_vecc;
// DESIGN.md section 5m) ----
// dot_block_kernel<K>, calc_r_block_kernel<K, false> and calc_px_block_kernel<K, false> on codewords: their grid, walk
// (one row per thread step), block_load / block_store and reduce_finish_k, every multiply and add separate.  A STEP is
// one row: all K columns of all operands, inactive columns included -- protection does not stop when a column
// converges.  The discipline is that of the single kernels above: a step with a suspect word is only noted -- nothing
// of it is stored or summed -- and behind the loop a thread with a noted step walks its chain once more.  There a
// step that reads clean has been carried out and adds the stored values it left; a step that still fails has every
// word decoded through vecc_cold (repair in registers, event with index row * K + column), is carried out and adds
// what it stores.  An active column is computed; an inactive one is selected, never computed with, and in a written
// operand its word is stored back as repaired: a clean word keeps every bit.  Per column the operations and roundings
// of calc_r_vecc_walk / calc_px_vecc_walk: column j is, word for word, what they leave for column j alone.

// bit 0: a word of the row fails its check
template <int K>
__device__ __forceinline__ uint32_t block_suspect(const double *v) {
  uint32_t sus = 0u;
#pragma unroll
  for (int j = 0; j < K; j++) sus |= vecc_suspect(vecc_bits(v[j]));
  return sus;
}

// the full decode of a word in a register -> the word as repaired (two flips: as it is)
__device__ __forceinline__ uint64_t vecc_repaired(double v, uint32_t index, uint32_t operand, const EventRing &ev) {
  uint64_t w = vecc_bits(v);
  if (__builtin_expect(vecc_suspect(w) != 0u, 0)) w = vecc_cold(w, index, operand, ev).w;
  return w;
}

// operands 0: a, 1: b; nothing is written
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void dot_block_vecc_kernel(const double *__restrict__ a,
                                                                    const double *__restrict__ b, int n,
                                                                    ReduceOutK out, EventRing ev) {
  __shared__ double s_w[8 * K];
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = 0.0;
  uint32_t bad = 0u;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  const long first = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x;
  for (long i = first; i < n; i += stride) {
    double av[K], bv[K];
    block_load<K>(a + i * K, av);
    block_load<K>(b + i * K, bv);
    const uint32_t sus = block_suspect<K>(av) | block_suspect<K>(bv);
    bad |= sus;
    if (!sus) {
#pragma unroll
      for (int j = 0; j < K; j++) acc[j] += vecc_value(vecc_bits(av[j])) * vecc_value(vecc_bits(bv[j]));
    }
  }
  if (__builtin_expect(bad != 0u, 0)) {  // nothing was stored: the whole chain again, with the repairs
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = 0.0;
#pragma unroll 1
    for (long i = first; i < n; i += stride) {
      double av[K], bv[K];
      block_load<K>(a + i * K, av);
      block_load<K>(b + i * K, bv);
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint32_t at = (uint32_t)(i * K + j);
        const double x = vecc_value(vecc_repaired(av[j], at, 0u, ev));
        acc[j] += x * vecc_value(vecc_repaired(bv[j], at, 1u, ev));
      }
    }
  }
  reduce_finish_k<K>(acc, out, s_w);
}

// R <- enc(val(R) - alpha_j val(W)) in the active columns; the K sums over the stored R of EVERY column, as
// calc_r_block_kernel sums them: dot_block_vecc_kernel(R, R) of the R it leaves, bit for bit.  W is not written back.
// (calc_r_block_vecc_walk: the one body of calc_r_block_vecc_kernel and calc_r_block_vecc_until_kernel.  alpha: K
// scalars, the kernel argument's array or the guarded kernel's own; op_*: the ordinal a repaired word of that operand
// is reported under, as in calc_r_vecc_walk; acc: the K sums, zero on entry)
template <int K>
__device__ __forceinline__ void calc_r_block_vecc_walk(double *__restrict__ r, const double *__restrict__ w,
                                                       const double *alpha, uint32_t active, int n, uint32_t op_r,
                                                       uint32_t op_w, const EventRing &ev, double *acc) {
  uint32_t bad = 0u;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  const long first = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x;
  for (long i = first; i < n; i += stride) {
    double rv[K], wv[K];
    block_load<K>(r + i * K, rv);
    block_load<K>(w + i * K, wv);
    const uint32_t sus = block_suspect<K>(rv) | block_suspect<K>(wv);
    bad |= sus;
    if (!sus) {
#pragma unroll
      for (int j = 0; j < K; j++) {
        const double rs = vecc_double(vecc_encode(vecc_value(vecc_bits(rv[j])) - alpha[j] * vecc_value(vecc_bits(wv[j]))));
        rv[j] = ((active >> j) & 1u) ? rs : rv[j];
        const double q = vecc_value(vecc_bits(rv[j]));
        acc[j] += q * q;
      }
      block_store<K>(r + i * K, rv);
    }
  }
  if (__builtin_expect(bad != 0u, 0)) {
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = 0.0;
#pragma unroll 1
    for (long i = first; i < n; i += stride) {
      double rv[K], wv[K];
      block_load<K>(r + i * K, rv);  // a step carried out above: what it stored
      block_load<K>(w + i * K, wv);
      if (block_suspect<K>(rv) | block_suspect<K>(wv)) {
#pragma unroll
        for (int j = 0; j < K; j++) {
          const uint32_t at = (uint32_t)(i * K + j);
          const uint64_t ro = vecc_repaired(rv[j], at, op_r, ev);
          const uint64_t wo = vecc_repaired(wv[j], at, op_w, ev);
          const uint64_t rs = vecc_encode(vecc_value(ro) - alpha[j] * vecc_value(wo));
          rv[j] = vecc_double(((active >> j) & 1u) ? rs : ro);
        }
        block_store<K>(r + i * K, rv);
      }
#pragma unroll
      for (int j = 0; j < K; j++) {
        const double q = vecc_value(vecc_bits(rv[j]));
        acc[j] += q * q;
      }
    }
  }
}

// X <- enc(val(X) + alpha_j val(P)) and P <- enc(val(R) + beta_j val(P)), both from the old P, in the active columns.
// R is not written back.
// (calc_px_block_vecc_walk: the one body of calc_px_block_vecc_kernel and calc_px_block_vecc_until_kernel)
template <int K>
__device__ __forceinline__ void calc_px_block_vecc_walk(double *__restrict__ x, double *__restrict__ p,
                                                        const double *__restrict__ r, const double *alpha,
                                                        const double *beta, uint32_t active, int n, uint32_t op_x,
                                                        uint32_t op_p, uint32_t op_r, const EventRing &ev) {
  uint32_t bad = 0u;
  const long stride = (long)gridDim.x * ABFT_BLOCK;
  const long first = (long)blockIdx.x * ABFT_BLOCK + threadIdx.x;
  for (long i = first; i < n; i += stride) {
    double xv[K], pv[K], rv[K];
    block_load<K>(x + i * K, xv);
    block_load<K>(p + i * K, pv);
    block_load<K>(r + i * K, rv);
    const uint32_t sus = block_suspect<K>(xv) | block_suspect<K>(pv) | block_suspect<K>(rv);
    bad |= sus;
    if (!sus) {
#pragma unroll
      for (int j = 0; j < K; j++) {
        const bool on = (active >> j) & 1u;
        const double po = vecc_value(vecc_bits(pv[j]));
        const double xs = vecc_double(vecc_encode(vecc_value(vecc_bits(xv[j])) + alpha[j] * po));
        const double ps = vecc_double(vecc_encode(vecc_value(vecc_bits(rv[j])) + beta[j] * po));
        xv[j] = on ? xs : xv[j];
        pv[j] = on ? ps : pv[j];
      }
      block_store<K>(x + i * K, xv);
      block_store<K>(p + i * K, pv);
    }
  }
  if (__builtin_expect(bad != 0u, 0)) {
#pragma unroll 1
    for (long i = first; i < n; i += stride) {
      double xv[K], pv[K], rv[K];
      block_load<K>(x + i * K, xv);
      block_load<K>(p + i * K, pv);
      block_load<K>(r + i * K, rv);
      if (!(block_suspect<K>(xv) | block_suspect<K>(pv) | block_suspect<K>(rv))) continue;  // carried out above
#pragma unroll
      for (int j = 0; j < K; j++) {
        const bool on = (active >> j) & 1u;
        const uint32_t at = (uint32_t)(i * K + j);
        const uint64_t xo = vecc_repaired(xv[j], at, op_x, ev);
        const uint64_t po = vecc_repaired(pv[j], at, op_p, ev);
        const uint64_t ro = vecc_repaired(rv[j], at, op_r, ev);
        const uint64_t xs = vecc_encode(vecc_value(xo) + alpha[j] * vecc_value(po));
        const uint64_t ps = vecc_encode(vecc_value(ro) + beta[j] * vecc_value(po));
        xv[j] = vecc_double(on ? xs : xo);
        pv[j] = vecc_double(on ? ps : po);
      }
      block_store<K>(x + i * K, xv);
      block_store<K>(p + i * K, pv);
    }
  }
}

// calc_r_block on protected vectors (operands 0: R, 1: W)
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_block_vecc_kernel(double *__restrict__ r,
                                                                       const double *__restrict__ w,
                                                                       BlockScalars alpha, uint32_t active, int n,
                                                                       ReduceOutK out, EventRing ev) {
  __shared__ double s_w[8 * K];
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = 0.0;
  calc_r_block_vecc_walk<K>(r, w, alpha.v, active, n, 0u, 1u, ev, acc);
  reduce_finish_k<K>(acc, out, s_w);
}

// calc_px_block on protected vectors (operands 0: X, 1: P, 2: R)
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_block_vecc_kernel(double *__restrict__ x, double *__restrict__ p,
                                                                        const double *__restrict__ r,
                                                                        BlockScalars alpha, BlockScalars beta,
                                                                        uint32_t active, int n, EventRing ev) {
  calc_px_block_vecc_walk<K>(x, p, r, alpha.v, beta.v, active, n, 0u, 1u, 2u, ev);
}

// The guarded forms (abft_hip_cg_block_vecc_iteration_until_dev): the heads and the tail of
// calc_r_block_until_kernel and calc_px_block_until_kernel (PRECOND = false) around the protected block walks; records
// and dev_pw are plain doubles outside any code.  Operands as the guarded entries count them: X 1, R 2, P 3, W 4 (0 is
// the SpMM's gathered P).  A launch with no live column touches no vector: it repairs nothing and reports nothing.
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_block_vecc_until_kernel(double *__restrict__ r,
                                                                             const double *__restrict__ w,
                                                                             const double *in, const double *pw,
                                                                             double threshold, double *alpha_out,
                                                                             int n, ReduceOutB out, EventRing ev) {
  __shared__ double s_w[8 * K];
  double alpha[K], acc[K] = {};
  const uint32_t active = guard_block_r_head<K>(in, pw, threshold, alpha_out, out, alpha);
  if (!active) return;
  calc_r_block_vecc_walk<K>(r, w, alpha, active, n, 2u, 4u, ev, acc);
  guard_block_r_tail<K, false>(acc, active, in, out, s_w);
}

template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_block_vecc_until_kernel(double *__restrict__ x,
                                                                              double *__restrict__ p,
                                                                              const double *__restrict__ r,
                                                                              const double *in, const double *out,
                                                                              double threshold, const double *alpha_ptr,
                                                                              int n, EventRing ev) {
  double alpha[K], beta[K];
  const uint32_t active = guard_block_px_head<K>(in, out, threshold, alpha_ptr, alpha, beta);
  if (!active) return;
  calc_px_block_vecc_walk<K>(x, p, r, alpha, beta, active, n, 1u, 3u, 2u, ev);
}

hipError_t launch_dot_block_vecc(const double *a, const double *b, int n, int k, const ReduceOutK &out, EventRing ev,
                                 hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) hipLaunchKernelGGL(dot_block_vecc_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, a, b, n, out, ev)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_r_block_vecc(double *r, const double *w, int n, int k, const BlockScalars &alpha,
                                    uint32_t active, const ReduceOutK &out, EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL(calc_r_block_vecc_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, alpha, active, n, out, ev)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_px_block_vecc(double *x, double *p, const double *r, int n, int k, const BlockScalars &alpha,
                                     const BlockScalars &beta, uint32_t active, EventRing ev, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K) \
  hipLaunchKernelGGL(calc_px_block_vecc_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, alpha, beta, active, n, ev)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_r_block_vecc_until(double *r, const double *w, const double *in, const double *pw,
                                          double threshold, double *alpha_out, int n, int k, const ReduceOutB &out,
                                          EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                                 \
  hipLaunchKernelGGL(calc_r_block_vecc_until_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, in, pw, threshold, \
                     alpha_out, n, out, ev)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_calc_px_block_vecc_until(double *x, double *p, const double *r, const double *in, const double *out,
                                           double threshold, const double *alpha_ptr, int n, int k, EventRing ev,
                                           hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                               \
  hipLaunchKernelGGL(calc_px_block_vecc_until_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, in, out, \
                     threshold, alpha_ptr, n, ev)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// ---- Jacobi preconditioning on protected vectors (abft_hip_precond_start_vecc, abft_hip_calc_r_precond_vecc,
// abft_hip_calc_px_precond_vecc) and the guarded iteration built on them (abft_hip_pcg_vecc_iteration_until_dev;
// DESIGN.md section 5l) ----
// The r / px cut above with z = dec(dinv) * (value of r), one rounded product that is never stored and never
// truncated, where the plain preconditioned kernels form it: p <- enc(z) at the start, {sum r z, sum r r} over the r
// the r half stores, p <- enc(z + beta dec(p)) in the x / p half.  dinv holds codewords like every other operand.
// Walks, grid, stride and per-thread sums are those of dot_vecc_kernel, calc_r_vecc_walk and calc_px_vecc_walk, VEC = 2
// when ALL operands of the call, dinv included, are 16-byte aligned; the two sums meet as precond_start_kernel's do.
// With dinv == enc(1.0) in every entry z is the value of r bit for bit, so r, x, p and r.r are the plain protected
// kernels' and r.z has r.r's bits.  Same cold-path discipline: a step with a suspect word is only noted and the chain
// walked once more behind the loop.  One exception to "a vector that is only read is not written back": dinv outlives
// the iteration -- no kernel ever rewrites it --, so the cold path stores a repaired dinv word back (the one lane that
// owns the element: a flip in dinv is reported once and gone afterwards; two flips stay, fatal).
// ONE body per pair (section 5i), the operand ordinals passed in as above: the two halves are vecc_walk with
// VeccCalcR<true> and VeccCalcPxPrecond, whose DINV operand is the one stored back; the start is written out (section 5p).

// vecc_decode_cold_ok for a dinv word: the repaired word is stored back
__device__ __forceinline__ double vecc_decode_cold_fix(double *p, uint32_t index, uint32_t operand, const EventRing &ev) {
  uint64_t w = vecc_bits(*p);
  if (__builtin_expect(vecc_suspect(w) != 0u, 0)) {
    const VeccWord o = vecc_cold(w, index, operand, ev);
    if (o.rc > 0) *p = vecc_double(o.w);
    w = o.w;
  }
  return vecc_value(w);
}

// (this walk keeps its hand-written form: under vecc_walk its VEC == 1 instance took two VGPRs more; section 5p)
// p <- enc(z), z = dec(dinv) * dec(r); acc += {sum dec(r) z, sum dec(r)^2}.  r is not written back, p only written.
template <int VEC>
__device__ __forceinline__ void precond_start_vecc_walk(const double *__restrict__ r, double *__restrict__ dinv,
                                                        double *__restrict__ p, int n, uint32_t op_r, uint32_t op_d,
                                                        EventRing ev, double *acc) {
  uint32_t bad = 0u;
  const long stride = (long)gridDim.x * ABFT_BLOCK * VEC;
  const long first = ((long)blockIdx.x * ABFT_BLOCK + threadIdx.x) * VEC;
  for (long i = first; i < n; i += stride) {
    if (VEC == 2 && i + 1 < n) {
      const double2 rv = *reinterpret_cast<const double2 *>(r + i);
      const double2 dv = *reinterpret_cast<const double2 *>(dinv + i);
      const uint64_t r0 = vecc_bits(rv.x), r1 = vecc_bits(rv.y), d0 = vecc_bits(dv.x), d1 = vecc_bits(dv.y);
      const uint32_t sus = (vecc_suspect(r0) | vecc_suspect(r1)) | (vecc_suspect(d0) | vecc_suspect(d1));
      bad |= sus;
      if (!sus) {
        const double z0 = vecc_value(d0) * vecc_value(r0), z1 = vecc_value(d1) * vecc_value(r1);
        *reinterpret_cast<double2 *>(p + i) = make_double2(vecc_double(vecc_encode(z0)), vecc_double(vecc_encode(z1)));
        acc[0] += vecc_value(r0) * z0;
        acc[0] += vecc_value(r1) * z1;
        acc[1] += vecc_value(r0) * vecc_value(r0);
        acc[1] += vecc_value(r1) * vecc_value(r1);
      }
    } else {
      const uint64_t r0 = vecc_bits(r[i]), d0 = vecc_bits(dinv[i]);
      const uint32_t sus = vecc_suspect(r0) | vecc_suspect(d0);
      bad |= sus;
      if (!sus) {
        const double z = vecc_value(d0) * vecc_value(r0);
        p[i] = vecc_double(vecc_encode(z));
        acc[0] += vecc_value(r0) * z;
        acc[1] += vecc_value(r0) * vecc_value(r0);
      }
    }
  }
  if (__builtin_expect(bad != 0u, 0)) {  // r and dinv are as they were, p is only written: the whole chain again
    acc[0] = 0.0; acc[1] = 0.0;
    for (long i = first; i < n; i += stride) {
      const int m = (VEC == 2 && i + 1 < n) ? 2 : 1;
      for (int k = 0; k < m; k++) {
        const uint32_t j = (uint32_t)(i + k);
        const double ro = vecc_decode_cold_ok(r + i + k, j, op_r, ev);
        const double z = vecc_decode_cold_fix(dinv + i + k, j, op_d, ev) * ro;
        p[i + k] = vecc_double(vecc_encode(z));
        acc[0] += ro * z;
        acc[1] += ro * ro;
      }
    }
  }
}

// r <- enc(dec(r) - alpha dec(w)); acc += {sum r' z', sum r' r'}, r' the stored r without its code bits and
// z' = dec(dinv) * r'.  w is not written back.
template <int VEC>
__device__ __forceinline__ void calc_r_precond_vecc_walk(double *__restrict__ r, const double *__restrict__ w,
                                                         double *__restrict__ dinv, double alpha, int n, uint32_t op_r,
                                                         uint32_t op_w, uint32_t op_d, EventRing ev, double *acc) {
  VeccColdDev cold{ev};
  vecc_grid_walk<VEC>(VeccCalcR<true>{alpha},
                      VeccOperands<VeccCalcR<true>>{{r, const_cast<double *>(w), dinv}, {op_r, op_w, op_d}}, n, cold, acc);
}

// x <- enc(dec(x) + alpha dec(p)) and p <- enc(dec(dinv) dec(r) + beta dec(p)) in one pass over p, both from the
// old p; r is not written back
template <int VEC>
__device__ __forceinline__ void calc_px_precond_vecc_walk(double *__restrict__ x, double *__restrict__ p,
                                                          const double *__restrict__ r, double *__restrict__ dinv,
                                                          double alpha, double beta, int n, uint32_t op_x,
                                                          uint32_t op_p, uint32_t op_r, uint32_t op_d, EventRing ev) {
  VeccColdDev cold{ev};
  vecc_grid_walk<VEC>(VeccCalcPxPrecond{alpha, beta},
                      VeccOperands<VeccCalcPxPrecond>{{x, p, const_cast<double *>(r), dinv}, {op_x, op_p, op_r, op_d}}, n,
                      cold, nullptr);
}

// p = enc(dinv r); {r.z, r.r} (operands 0: r, 1: dinv, 2: p)
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void precond_start_vecc_kernel(const double *__restrict__ r,
                                                                        double *__restrict__ dinv,
                                                                        double *__restrict__ p, int n, ReduceOutK out,
                                                                        EventRing ev) {
  __shared__ double s_w[16];
  double acc[2] = {0.0, 0.0};
  precond_start_vecc_walk<VEC>(r, dinv, p, n, 0u, 1u, ev, acc);
  reduce_finish_k<2>(acc, out, s_w);
}

// r -= alpha w; {r.z, r.r} of the r it stores (operands 0: r, 1: w, 2: dinv)
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_precond_vecc_kernel(double *__restrict__ r,
                                                                         const double *__restrict__ w,
                                                                         double *__restrict__ dinv, double alpha, int n,
                                                                         ReduceOutK out, EventRing ev) {
  __shared__ double s_w[16];
  double acc[2] = {0.0, 0.0};
  calc_r_precond_vecc_walk<VEC>(r, w, dinv, alpha, n, 0u, 1u, 2u, ev, acc);
  reduce_finish_k<2>(acc, out, s_w);
}

// x += alpha p; p = dinv r + beta p (operands 0: x, 1: p, 2: r, 3: dinv)
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_precond_vecc_kernel(double *__restrict__ x, double *__restrict__ p,
                                                                          const double *__restrict__ r,
                                                                          double *__restrict__ dinv, double alpha,
                                                                          double beta, int n, EventRing ev) {
  calc_px_precond_vecc_walk<VEC>(x, p, r, dinv, alpha, beta, n, 0u, 1u, 2u, 3u, ev);
}

// The guarded forms: calc_r_precond_until_kernel and calc_px_precond_until_kernel with the protected walks.  Operands
// as the guarded entry counts them: x 1, r 2, p 3, w 4, dinv 5 (0 is the SpMV's gathered vector).  A frozen launch
// touches no vector, dinv included: it repairs nothing and reports nothing.
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_precond_vecc_until_kernel(double *__restrict__ r,
                                                                               const double *__restrict__ w,
                                                                               double *__restrict__ dinv,
                                                                               const double *in, const double *pw,
                                                                               double threshold, double *alpha_out,
                                                                               int n, ReduceOutD out, EventRing ev) {
  __shared__ double s_w[16];
  double alpha;
  if (!guard_r_head<GuardQuad>(in, pw, threshold, alpha_out, out, &alpha)) return;
  double acc[2] = {0.0, 0.0};
  calc_r_precond_vecc_walk<VEC>(r, w, dinv, alpha, n, 2u, 4u, 5u, ev, acc);
  reduce_finish_d(acc, out, s_w);
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_precond_vecc_until_kernel(double *__restrict__ x,
                                                                                double *__restrict__ p,
                                                                                const double *__restrict__ r,
                                                                                double *__restrict__ dinv,
                                                                                const double *in, const double *out,
                                                                                double threshold,
                                                                                const double *alpha_ptr, int n,
                                                                                EventRing ev) {
  if (!GuardQuad::live(in, threshold)) return;
  const double beta = GuardQuad::beta(in, out);
  const double alpha = *alpha_ptr;
  calc_px_precond_vecc_walk<VEC>(x, p, r, dinv, alpha, beta, n, 1u, 3u, 2u, 5u, ev);
}

// (each chooses its walk over its own operands, in the host-scalar and in the guarded form alike)
hipError_t launch_precond_start_vecc(const double *r, double *dinv, double *p, int n, const ReduceOutK &out,
                                     EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(precond_start_vecc_kernel, (), aligned16(r, dinv, p), nb, r, dinv, p, n, out, ev);
  return hipGetLastError();
}

hipError_t launch_calc_r_precond_vecc(double *r, const double *w, double *dinv, double alpha, int n,
                                      const ReduceOutK &out, EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_r_precond_vecc_kernel, (), aligned16(r, w, dinv), nb, r, w, dinv, alpha, n, out, ev);
  return hipGetLastError();
}

hipError_t launch_calc_px_precond_vecc(double *x, double *p, const double *r, double *dinv, double alpha, double beta,
                                       int n, EventRing ev, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_px_precond_vecc_kernel, (), aligned16(x, p, r, dinv), nb, x, p, r, dinv, alpha, beta, n, ev);
  return hipGetLastError();
}

hipError_t launch_calc_r_precond_vecc_until(double *r, const double *w, double *dinv, const double *in,
                                            const double *pw, double threshold, double *alpha_out, int n,
                                            const ReduceOutD &out, EventRing ev, hipStream_t s) {
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_r_precond_vecc_until_kernel, (), aligned16(r, w, dinv), nb, r, w, dinv, in, pw, threshold,
                    alpha_out, n, out, ev);
  return hipGetLastError();
}

hipError_t launch_calc_px_precond_vecc_until(double *x, double *p, const double *r, double *dinv, const double *in,
                                             const double *out, double threshold, const double *alpha_ptr, int n,
                                             EventRing ev, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  ABFT_VEC_DISPATCH(calc_px_precond_vecc_until_kernel, (), aligned16(x, p, r, dinv), nb, x, p, r, dinv, in, out,
                    threshold, alpha_ptr, n, ev);
  return hipGetLastError();
}

// ------------------------------------------------------------ the protected trail --
// The guarded iteration on a trail of SECDED slots (trail_ecc.h): siblings of the fold kernels
// and of the eight guarded halves above, with symbols of their own, so that no instantiation of those moves.  The
// walks, block_sum, the ticket protocol and the fixed-order folds are the unprotected kernels' own bodies; what
// differs is the head -- every slot a launch reads is checked -- and the publication, which writes slots.
// Reduction partials and tickets stay plain: they are written and consumed inside one iteration.
//
// A slot is read by every thread of a launch, uniformly.  Its one OWNER per launch is thread 0 of workgroup 0: all
// repair a flipped bit in their registers, the owner alone stores the clean slot back (a plain store) and queues the
// event.  A workgroup that loads behind the store-back sees the clean word and decodes the same value.

struct TrailGot { uint64_t bits; int rc; };  // the value of a slot; rc 0 clean, 1 repaired, -1 two flips

__device__ __noinline__ TrailGot trail_cold(uint4 d, uint4 *at, uint32_t ordinal, uint32_t record, bool owner,
                                            EventRing ev) {
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  const TrailWord t = trail_decode_at(w, ordinal);  // (a codeword of another ordinal, or word 1 set: as two flips)
  if (owner && t.rc) {
    if (t.rc > 0) *at = make_uint4(t.w[0], t.w[1], t.w[2], t.w[3]);
    push_event(ev, t.rc > 0 ? ABFT_EV_TRAIL_CORRECTED : ABFT_EV_TRAIL_DOUBLE, ordinal,
               (t.rc > 0 ? t.bit : 0u) | (record << 8), ABFT_FMT_CSR);
  }
  return TrailGot{t.bits, t.rc};
}

// slot `ordinal` of the record at rec (16-byte aligned: the entries check it), checked
__device__ __forceinline__ TrailGot trail_get(double *rec, int ordinal, uint32_t record, bool owner, EventRing ev) {
  uint4 *at = reinterpret_cast<uint4 *>(rec) + ordinal;
  const uint4 d = *at;  // uniform, 16 bytes
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  if (__builtin_expect((blk_suspect(w) | trail_misplaced(w, (uint32_t)ordinal)) != 0u, 0))
    return trail_cold(d, at, (uint32_t)ordinal, record, owner, ev);
  return TrailGot{trail_bits(w), 0};
}

// The head of every r half on a protected trail (T: TrailPair, TrailQuad): true -> live, with alpha.  false -> the
// launch ends here, before it touches a vector, a partial or the ticket: frozen, the record handed on repaired and
// re-encoded by the owner; or two flips in a slot the decision depends on, the record handed on word for word.
template <class T>
__device__ __forceinline__ bool trail_r_head(double *in, double *pw, double threshold, double *out, const uint32_t *ev_count,
                                             EventRing ev, double *alpha) {
  const bool owner = blockIdx.x == 0 && threadIdx.x == 0;
  const TrailGot rr = trail_get(in, T::RR, ABFT_TRAIL_START, owner, ev);
  TrailGot rz = rr;
  if (T::RZ != T::RR && rr.rc >= 0) rz = trail_get(in, T::RZ, ABFT_TRAIL_START, owner, ev);
  if (rr.rc < 0 || rz.rc < 0) {
    if (owner) T::hand_on_raw(in, out);
    return false;
  }
  if (!T::live(rr.bits, threshold)) {
    if (owner) T::hand_on(rr.bits, rz.bits, out, __hip_atomic_load(ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return false;
  }
  const TrailGot pv = trail_get(pw, 0, ABFT_TRAIL_PW, owner, ev);
  if (pv.rc < 0) {
    if (owner) T::hand_on_raw(in, out);
    return false;
  }
  *alpha = T::alpha(rr.bits, rz.bits, pv.bits);
  return true;
}

// The head of every x / p half: true -> live, with alpha -- formed from the same two checked slots as the r half's,
// the same IEEE quotient: there is no alpha scratch word -- and beta.  false: frozen, or two flips in a slot the
// decision depends on (the new record's r.z among them): x and p keep every bit.
template <class T>
__device__ __forceinline__ bool trail_px_head(double *in, double *pw, double *out, double threshold, EventRing ev,
                                              double *alpha, double *beta) {
  const bool owner = blockIdx.x == 0 && threadIdx.x == 0;
  const TrailGot rr = trail_get(in, T::RR, ABFT_TRAIL_START, owner, ev);
  if (rr.rc < 0 || !T::live(rr.bits, threshold)) return false;
  TrailGot rz = rr;
  if (T::RZ != T::RR) rz = trail_get(in, T::RZ, ABFT_TRAIL_START, owner, ev);
  if (rz.rc < 0) return false;
  const TrailGot pv = trail_get(pw, 0, ABFT_TRAIL_PW, owner, ev);
  if (pv.rc < 0) return false;
  const TrailGot nz = trail_get(out, T::RZ, ABFT_TRAIL_NEXT, owner, ev);
  if (nz.rc < 0) return false;
  *alpha = T::alpha(rr.bits, rz.bits, pv.bits);
  *beta = T::beta(rr.bits, rz.bits, nz.bits);
  return true;
}

// reduce_finish with the pair {sum, queued events} published as slots (no peers, no pinned slot: one rank, device
// scalars): the partial stores, the ticket and the last arriver's fixed-order fold are reduce_finish's
__device__ __forceinline__ void reduce_finish_trail(double block_value, const ReduceOut &o, double *s_w) {
  __shared__ uint32_t s_last;
  if (threadIdx.x == 0) {
    __hip_atomic_store(o.partials + blockIdx.x, block_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = reduce_take_ticket(o.ticket);
  }
  __syncthreads();
  if (!s_last) return;
  const double acc = fold_block_partials<true>(o.partials, gridDim.x, s_w);
  if (threadIdx.x == 0) {
    const uint32_t nev = reduce_rearm(o);
    TrailPair::publish(acc, acc, o.dev_out, nev);
  }
}

// reduce_finish_d with the record {r.r, queued events, r.z, 0.0} published as slots
__device__ __forceinline__ void reduce_finish_d_trail(const double *value, const ReduceOutD &o, double *s_w) {
  double tot[2];
  if (!reduce_totals_k<2>(value, o, s_w, tot) || threadIdx.x != 0) return;
  const uint32_t nev = reduce_rearm(o);
  TrailQuad::publish(tot[1], tot[0], o.dev_out, nev);
}

// ---- the folds of the SpMV's fused product: fuse_finalize_kernel and fold_partials_kernel, {p.w, events} as slots ----
// (fuse_finalize_kernel's sum is restated here, line for line -- the same order and shape, so the same bits, which the
// clean-parity tests hold --: sharing one inlined body moved an instruction of that kernel)
__global__ __launch_bounds__(1024) void fuse_finalize_trail_kernel(FuseOut f, uint32_t nblk, FixArgs fx) {
  __shared__ double s_w[16];
  if (fx.on) coo_fixup_body(fx);
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < nblk; i += 16u * 1024u) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const uint32_t j = i + (uint32_t)k * 1024u;
      v[k] = j < nblk ? f.partials[j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 16; k += 4) acc += (v[k] + v[k + 1]) + (v[k + 2] + v[k + 3]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < 16; k++) tot += s_w[k];
    TrailPair::publish_pw(tot, f.dev_out, *f.ev_count);
  }
}

__global__ __launch_bounds__(ABFT_BLOCK) void fold_partials_trail_kernel(const double *__restrict__ parts, uint32_t n,
                                                                         uint32_t chunk, ReduceOut out, FixArgs fx) {
  __shared__ double s_w[4];
  if (fx.on && blockIdx.x == 0) coo_fixup_body(fx);
  const uint32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  double acc = fold_chunk_sum(parts, lo, hi);
  acc = block_sum(acc, s_w);
  reduce_finish_trail(acc, out, s_w);
}

// launch_fuse_finalize's rule: one workgroup up to 8192 partials, the multi-workgroup fold above
hipError_t launch_fuse_finalize_trail(const FuseOut &f, uint32_t nblk, const ReduceOut &big, const FixArgs *fix,
                                      hipStream_t s) {
  FixArgs fx{};
  if (fix) fx = *fix;
  if (!fuse_finalize_folds(nblk) || !big.partials) {
    hipLaunchKernelGGL(fuse_finalize_trail_kernel, dim3(1), dim3(1024), 0, s, f, nblk, fx);
    return hipGetLastError();
  }
  uint32_t chunk;
  const uint32_t nb = fold_grid(nblk, &chunk);
  hipLaunchKernelGGL(fold_partials_trail_kernel, dim3(nb), dim3(ABFT_BLOCK), 0, s, f.partials, nblk, chunk, big, fx);
  return hipGetLastError();
}

// ---- the eight guarded halves ----
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_trail_until_kernel(double *r, const double *__restrict__ w,
                                                                        TrailIter t, int n, ReduceOut out) {
  __shared__ double s_w[4];
  double alpha;
  if (!trail_r_head<TrailPair>(t.in, t.pw, t.threshold, t.out, out.ev_count, t.ev, &alpha)) return;
  double acc = calc_r_walk<VEC>(r, w, alpha, n, r);
  acc = block_sum(acc, s_w);
  reduce_finish_trail(acc, out, s_w);
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_trail_until_kernel(double *p, const double *__restrict__ r,
                                                                         double *x, TrailIter t, int n) {
  double alpha, beta;
  if (!trail_px_head<TrailPair>(t.in, t.pw, t.out, t.threshold, t.ev, &alpha, &beta)) return;
  calc_px_walk<VEC>(p, r, x, beta, alpha, n, p, x);
}

template <int VEC, bool PAIRS>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_precond_trail_until_kernel(double *r, const double *w,
                                                                                const double *__restrict__ dinv,
                                                                                TrailIter t, int n, ReduceOutD out) {
  __shared__ double s_w[16];
  double alpha;
  if (!trail_r_head<TrailQuad>(t.in, t.pw, t.threshold, t.out, out.ev_count, t.ev, &alpha)) return;
  double acc[2] = {0.0, 0.0};
  calc_xr_precond_walk<VEC, PAIRS, false>(nullptr, r, nullptr, w, dinv, alpha, n, acc);
  reduce_finish_d_trail(acc, out, s_w);
}

template <int VEC, bool PAIRS>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_precond_trail_until_kernel(double *__restrict__ p,
                                                                                 const double *__restrict__ r,
                                                                                 const double *__restrict__ dinv,
                                                                                 double *__restrict__ x, TrailIter t,
                                                                                 int n) {
  double alpha, beta;
  if (!trail_px_head<TrailQuad>(t.in, t.pw, t.out, t.threshold, t.ev, &alpha, &beta)) return;
  calc_p_precond_walk<VEC, PAIRS, true>(p, r, dinv, x, beta, alpha, n);
}

// on protected vectors: operands as the guarded entries count them (x 1, r 2, p 3, w 4, dinv 5)
template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_vecc_trail_until_kernel(double *__restrict__ r,
                                                                             const double *__restrict__ w, TrailIter t,
                                                                             int n, ReduceOut out) {
  __shared__ double s_w[4];
  double alpha;
  if (!trail_r_head<TrailPair>(t.in, t.pw, t.threshold, t.out, out.ev_count, t.ev, &alpha)) return;
  double acc = calc_r_vecc_walk<VEC>(r, w, alpha, n, 2u, 4u, t.ev);
  acc = block_sum(acc, s_w);
  reduce_finish_trail(acc, out, s_w);
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_vecc_trail_until_kernel(double *__restrict__ x,
                                                                              double *__restrict__ p,
                                                                              const double *__restrict__ r, TrailIter t,
                                                                              int n) {
  double alpha, beta;
  if (!trail_px_head<TrailPair>(t.in, t.pw, t.out, t.threshold, t.ev, &alpha, &beta)) return;
  calc_px_vecc_walk<VEC>(x, p, r, alpha, beta, n, 1u, 3u, 2u, t.ev);
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_precond_vecc_trail_until_kernel(double *__restrict__ r,
                                                                                     const double *__restrict__ w,
                                                                                     double *__restrict__ dinv,
                                                                                     TrailIter t, int n,
                                                                                     ReduceOutD out) {
  __shared__ double s_w[16];
  double alpha;
  if (!trail_r_head<TrailQuad>(t.in, t.pw, t.threshold, t.out, out.ev_count, t.ev, &alpha)) return;
  double acc[2] = {0.0, 0.0};
  calc_r_precond_vecc_walk<VEC>(r, w, dinv, alpha, n, 2u, 4u, 5u, t.ev, acc);
  reduce_finish_d_trail(acc, out, s_w);
}

template <int VEC>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_precond_vecc_trail_until_kernel(double *__restrict__ x,
                                                                                      double *__restrict__ p,
                                                                                      const double *__restrict__ r,
                                                                                      double *__restrict__ dinv,
                                                                                      TrailIter t, int n) {
  double alpha, beta;
  if (!trail_px_head<TrailQuad>(t.in, t.pw, t.out, t.threshold, t.ev, &alpha, &beta)) return;
  calc_px_precond_vecc_walk<VEC>(x, p, r, dinv, alpha, beta, n, 1u, 3u, 2u, 5u, t.ev);
}

// The r half.  VEC (and PAIRS) as the unprotected guarded launcher of the same loop chooses them, so that the sums
// are added in the same order.  o: the pair loops' reduction, od: the record loops'.
hipError_t launch_trail_r_until(bool vecc, bool precond, double *r, const double *w, double *dinv, const double *x,
                                const double *p, const TrailIter &t, int n, const ReduceOut &o, const ReduceOutD &od,
                                hipStream_t s) {
  const int nb = reduce_blocks(n);
  if (vecc && precond)
    ABFT_VEC_DISPATCH(calc_r_precond_vecc_trail_until_kernel, (), aligned16(r, w, dinv), nb, r, w, dinv, t, n, od);
  else if (vecc)
    ABFT_VEC_DISPATCH(calc_r_vecc_trail_until_kernel, (), aligned16(r, w), nb, r, w, t, n, o);
  else if (precond) {
    const bool vec2 = aligned16(r, w), pairs = aligned16(dinv);
    ABFT_PRECOND_DISPATCH(calc_r_precond_trail_until_kernel, (), r, w, dinv, t, n, od);
  } else
    ABFT_VEC_DISPATCH(calc_r_trail_until_kernel, (), aligned16(r, w, x, p), nb, r, w, t, n, o);
  return hipGetLastError();
}

hipError_t launch_trail_px_until(bool vecc, bool precond, double *x, double *p, const double *r, double *dinv,
                                 const TrailIter &t, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
  if (vecc && precond)
    ABFT_VEC_DISPATCH(calc_px_precond_vecc_trail_until_kernel, (), aligned16(x, p, r, dinv), nb, x, p, r, dinv, t, n);
  else if (vecc)
    ABFT_VEC_DISPATCH(calc_px_vecc_trail_until_kernel, (), aligned16(x, p, r), nb, x, p, r, t, n);
  else if (precond) {
    const bool vec2 = aligned16(p, r, x), pairs = aligned16(dinv);
    ABFT_PRECOND_DISPATCH(calc_px_precond_trail_until_kernel, (), p, r, dinv, x, t, n);
  } else
    ABFT_VEC_DISPATCH(calc_px_trail_until_kernel, (), aligned16(p, r, x), nb, p, r, x, t, n);
  return hipGetLastError();
}
#undef ABFT_PRECOND_DISPATCH

// ---- the guarded block iteration on a protected trail ----
// spmm_fold_dev_kernel<K>, calc_r_block_until_kernel<K, PRECOND>, calc_px_block_until_kernel<K, PRECOND> and the two
// protected-vector halves on TrailBlock<K> slots (trail_ecc.h): symbols of their own again.  fold_chunk_sum, the four
// block walks, reduce_totals_k and the ticket are the unprotected kernels' bodies; the heads read slots through
// trail_get and the publications write slots.  What a launch reads is TrailBlock's read_start / read_scalars: all 2K
// value slots of the start record; of a live launch P.W[j] -- in the x / p half also the next record's r.z[j] -- of
// the live columns only.  No alpha scratch: both halves form alpha_j from the same two checked slots.

// trail_get as TrailBlock's reader: (record, ordinal) -> the checked slot of that record, owning nothing (the tail)
struct TrailBlockGet {
  double *in, *pw, *out;
  EventRing ev;
  __device__ __forceinline__ TrailGot operator()(uint32_t record, int ordinal) const {
    return trail_get(record == ABFT_TRAIL_START ? in : record == ABFT_TRAIL_PW ? pw : out, ordinal, record, false, ev);
  }
};

// The heads spread their slots over the lanes of every wave: ONE LANE, ONE SLOT.  Lane l loads and checks the slot of
// ordinal l -- the hot test, and trail_cold for the lanes whose slot fails it --, so that all slots of a phase are in
// flight at once and a head holds four words a lane whatever K is (read one after the other by every thread, the 2K
// to 4K checked slots of a K = 8 head cost the walks behind them their occupancy).  The values then go to every lane
// through readlane, into scalar registers, and TrailBlock's rules run on them: the decision is uniform over the
// wave, and over the grid because every wave decodes the same words.  Each slot keeps one owner per launch: the lane
// that reads it in wave 0 of workgroup 0 stores a repair back and queues the event.
struct TrailLane { uint64_t bits; int rc; };  // what a lane holds of its slot (a lane without one: 0, clean)

__device__ __forceinline__ TrailLane trail_lane_get(bool want, double *rec, int ordinal, uint32_t record, bool owner,
                                                    EventRing ev) {
  TrailLane g{0u, 0};
  if (want) {
    const TrailGot t = trail_get(rec, ordinal, record, owner, ev);
    g.bits = t.bits;
    g.rc = t.rc;
  }
  return g;
}

// TrailBlock's reader over the lanes: the slot of ordinal o sits in lane o -- the start record's 2K values in lanes
// 0 .. 2K - 1; then P.W[j] in lane j and the next record's r.z[j], whose ordinal is K + j, in lane K + j
struct TrailLaneGet {
  TrailLane lane;
  __device__ __forceinline__ TrailGot operator()(uint32_t, int ordinal) const {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)lane.bits, ordinal);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(lane.bits >> 32), ordinal);
    return TrailGot{(uint64_t)lo | ((uint64_t)hi << 32), __builtin_amdgcn_readlane(lane.rc, ordinal)};
  }
};

// spmm_fold_dev_kernel<K> with the last arriver publishing {P.W[K], queued events} as K + 1 fresh slots
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void spmm_fold_trail_kernel(const double *__restrict__ parts, uint32_t n,
                                                                     uint32_t chunk, ReduceOutB out) {
  __shared__ double s_w[8 * K];
  const uint32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  double acc[K], tot[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = fold_chunk_sum(parts + (size_t)j * n, lo, hi);
  if (!reduce_totals_k<K, ReduceOutB, uint32_t>(acc, out, s_w, tot)) return;
  if (threadIdx.x == 0) {
    const uint32_t nev = reduce_rearm(out);
    TrailBlock<K>::publish_pw(tot, out.dev_out, nev);
  }
}

hipError_t launch_spmm_fold_trail(const double *parts, uint32_t nblk, int k, const ReduceOutB &out, hipStream_t s) {
  uint32_t chunk;
  const uint32_t nb = fold_grid(nblk, &chunk);  // launch_spmm_fold's grid and chunks
#define ABFT_OP(K) hipLaunchKernelGGL(spmm_fold_trail_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, parts, nblk, chunk, out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// The head of the r half -> the mask, uniform over the grid, and the K alphas (a frozen column's:
// +0.0, which the walk's select drops).  0: the launch ends here, before it touches a vector, a partial or the
// ticket -- no column live, the record handed on repaired and re-encoded by the owner; or two flips in a slot read,
// the record handed on word for word.  (noescape: as guard_block_r_head)
template <int K>
__device__ __forceinline__ uint32_t trail_block_r_head(const TrailIter &t, const uint32_t *ev_count,
                                                       double *alpha __attribute__((noescape))) {
  using T = TrailBlock<K>;
  const bool owner = blockIdx.x == 0 && threadIdx.x == 0, own = blockIdx.x == 0 && threadIdx.x < 64u;
  const int lane = (int)(threadIdx.x & 63u);
  const TrailLane start = trail_lane_get(lane < T::VALUES, t.in, lane, ABFT_TRAIL_START, own, t.ev);
  uint64_t v[T::VALUES];
  if (!T::read_start(TrailLaneGet{start}, v)) {
    if (owner) T::hand_on_raw(t.in, t.out);
    return 0u;
  }
  const uint32_t active = (uint32_t)__builtin_amdgcn_readfirstlane((int)T::live_mask(v, t.threshold));
  if (!active) {
    if (owner) T::hand_on(v, t.out, __hip_atomic_load(ev_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return 0u;
  }
  const TrailLane live = trail_lane_get(lane < K && ((active >> (lane & 31)) & 1u), t.pw, lane, ABFT_TRAIL_PW, own, t.ev);
  if (!T::template read_scalars<false>(TrailLaneGet{live}, v, active, alpha, nullptr)) {
    if (owner) T::hand_on_raw(t.in, t.out);
    return 0u;
  }
  return active;
}

// The K scalars of a live launch into scalar registers, as guard_block_r_head has them.  The kernels do this behind
// their `if (!active) return`: done inside the heads, the paths that return 0 with some scalars already formed meet
// the live path first, and the compiler keeps all of them in vector registers across the walk.
template <int K>
__device__ __forceinline__ void trail_block_uniform(double *s __attribute__((noescape))) {
#pragma unroll
  for (int j = 0; j < K; j++) s[j] = uniform_f64(s[j]);
}

// The tail: the sums meet as in guard_block_r_tail; the last block's first thread decodes the start record's value
// slots again -- owning nothing: no store, no event; a slot the head repaired decodes to the same bits whether or not
// the owner's store-back is visible yet -- and publishes slots.  (Decoded again instead of kept: 4K registers that
// would otherwise live across the walk.)
template <int K, bool PRECOND>
__device__ __forceinline__ void trail_block_r_tail(const double *acc, uint32_t active, const TrailIter &t,
                                                   const ReduceOutB &out, double *s_w) {
  constexpr int S = PRECOND ? 2 * K : K;
  double tot[S];
  if (!reduce_totals_k<S, ReduceOutB, uint32_t>(acc, out, s_w, tot) || threadIdx.x != 0) return;
  uint64_t v[TrailBlock<K>::VALUES];
  TrailBlock<K>::read_start(TrailBlockGet{t.in, t.pw, t.out, t.ev}, v);
  TrailBlock<K>::template publish<PRECOND>(tot, active, v, out.dev_out, reduce_rearm(out));
}

// The head of the x / p half -> the mask, and when it is not 0 the K alphas and betas.  0: nothing live, or two flips
// in a slot read (the next record's r.z of a live column among them): X and P keep every bit.
template <int K>
__device__ __forceinline__ uint32_t trail_block_px_head(const TrailIter &t, double *alpha __attribute__((noescape)),
                                                        double *beta __attribute__((noescape))) {
  using T = TrailBlock<K>;
  const bool own = blockIdx.x == 0 && threadIdx.x < 64u;
  const int lane = (int)(threadIdx.x & 63u);
  const TrailLane start = trail_lane_get(lane < T::VALUES, t.in, lane, ABFT_TRAIL_START, own, t.ev);
  uint64_t v[T::VALUES];
  if (!T::read_start(TrailLaneGet{start}, v)) return 0u;
  const uint32_t active = (uint32_t)__builtin_amdgcn_readfirstlane((int)T::live_mask(v, t.threshold));
  if (!active) return 0u;
  const bool tail = lane < K;  // lanes 0 .. K - 1: P.W[lane]; lanes K .. 2K - 1: the next record's r.z[lane - K]
  const bool want = lane < T::VALUES && ((active >> ((tail ? lane : lane - K) & 31)) & 1u);
  const TrailLane live = trail_lane_get(want, tail ? t.pw : t.out, lane, tail ? ABFT_TRAIL_PW : ABFT_TRAIL_NEXT, own, t.ev);
  if (!T::template read_scalars<true>(TrailLaneGet{live}, v, active, alpha, beta)) return 0u;
  return active;
}

template <int K, bool PRECOND>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_block_trail_until_kernel(double *__restrict__ r,
                                                                              const double *__restrict__ w,
                                                                              const double *__restrict__ dinv,
                                                                              TrailIter t, int n, ReduceOutB out) {
  constexpr int S = PRECOND ? 2 * K : K;
  __shared__ double s_w[8 * S];
  double alpha[K], acc[S] = {};
  const uint32_t active = trail_block_r_head<K>(t, out.ev_count, alpha);
  if (!active) return;
  trail_block_uniform<K>(alpha);
  calc_r_block_walk<K, PRECOND>(r, w, dinv, alpha, active, n, acc);
  trail_block_r_tail<K, PRECOND>(acc, active, t, out, s_w);
}

template <int K, bool PRECOND>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_block_trail_until_kernel(double *__restrict__ x,
                                                                               double *__restrict__ p,
                                                                               const double *__restrict__ r,
                                                                               const double *__restrict__ dinv,
                                                                               TrailIter t, int n) {
  double alpha[K], beta[K];
  const uint32_t active = trail_block_px_head<K>(t, alpha, beta);
  if (!active) return;
  trail_block_uniform<K>(alpha);
  trail_block_uniform<K>(beta);
  calc_px_block_walk<K, PRECOND>(x, p, r, dinv, alpha, beta, active, n);
}

// on protected block vectors: operands X 1, R 2, P 3, W 4, as calc_r_block_vecc_until_kernel counts them
template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_r_block_vecc_trail_until_kernel(double *__restrict__ r,
                                                                                   const double *__restrict__ w,
                                                                                   TrailIter t, int n, ReduceOutB out) {
  __shared__ double s_w[8 * K];
  double alpha[K], acc[K] = {};
  const uint32_t active = trail_block_r_head<K>(t, out.ev_count, alpha);
  if (!active) return;
  trail_block_uniform<K>(alpha);
  calc_r_block_vecc_walk<K>(r, w, alpha, active, n, 2u, 4u, t.ev, acc);
  trail_block_r_tail<K, false>(acc, active, t, out, s_w);
}

template <int K>
__global__ __launch_bounds__(ABFT_BLOCK) void calc_px_block_vecc_trail_until_kernel(double *__restrict__ x,
                                                                                    double *__restrict__ p,
                                                                                    const double *__restrict__ r,
                                                                                    TrailIter t, int n) {
  double alpha[K], beta[K];
  const uint32_t active = trail_block_px_head<K>(t, alpha, beta);
  if (!active) return;
  trail_block_uniform<K>(alpha);
  trail_block_uniform<K>(beta);
  calc_px_block_vecc_walk<K>(x, p, r, alpha, beta, active, n, 1u, 3u, 2u, t.ev);
}

// out.dev_out is t.out.  dinv == nullptr: the plain form; vecc: codewords (no dinv)
hipError_t launch_block_trail_r_until(bool vecc, double *r, const double *w, const double *dinv, const TrailIter &t,
                                      int n, int k, const ReduceOutB &out, hipStream_t s) {
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                                     \
  if (vecc)                                                                                                            \
    hipLaunchKernelGGL(calc_r_block_vecc_trail_until_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, t, n, out);    \
  else if (dinv)                                                                                                       \
    hipLaunchKernelGGL((calc_r_block_trail_until_kernel<K, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, dinv, t, n, \
                       out);                                                                                           \
  else                                                                                                                 \
    hipLaunchKernelGGL((calc_r_block_trail_until_kernel<K, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, r, w, dinv, t, n, \
                       out)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

hipError_t launch_block_trail_px_until(bool vecc, double *x, double *p, const double *r, const double *dinv,
                                       const TrailIter &t, int n, int k, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int nb = reduce_blocks(n);
#define ABFT_OP(K)                                                                                                     \
  if (vecc)                                                                                                            \
    hipLaunchKernelGGL(calc_px_block_vecc_trail_until_kernel<K>, dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, t, n);     \
  else if (dinv)                                                                                                       \
    hipLaunchKernelGGL((calc_px_block_trail_until_kernel<K, true>), dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, dinv, t, \
                       n);                                                                                             \
  else                                                                                                                 \
    hipLaunchKernelGGL((calc_px_block_trail_until_kernel<K, false>), dim3(nb), dim3(ABFT_BLOCK), 0, s, x, p, r, dinv, t, \
                       n)
  ABFT_BLOCK_K_DISPATCH(ABFT_OP)
#undef ABFT_OP
  return hipGetLastError();
}

// XOR `mask` into one stored slot (fault injection into the trail: tests and the CLI's --flip-trail)
__global__ void flip_trail_kernel(uint4 *slot, uint4 mask) {
  const uint4 d = *slot;
  *slot = make_uint4(d.x ^ mask.x, d.y ^ mask.y, d.z ^ mask.z, d.w ^ mask.w);
}

hipError_t launch_flip_trail(double *slot, const uint32_t mask[4], hipStream_t s) {
  hipLaunchKernelGGL(flip_trail_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<uint4 *>(slot),
                     make_uint4(mask[0], mask[1], mask[2], mask[3]));
  return hipGetLastError();
}
