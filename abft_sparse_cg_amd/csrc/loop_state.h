// loop_state.h -- what the library keeps between the calls of the host-scalar CG loop
//     rr = dot(r, r);  loop: spmv(A, p, w), pw = dot(p, w), rr' = calc_xr(x, r, p, w, rr / pw), calc_p(p, r, rr' / rr)
// and every decision taken on it: which call is served from what is already in flight, what is dropped, what is armed.
// Host code only, no HIP header: abft_hip.hip asks a decision here, does the GPU work (launches, allocations, waits
// for a pinned slot) and reports back through a transition; tests/host/loop_state_play.cpp does the same with no GPU.
// Nothing here launches, allocates or fails.  DESIGN.md section 4 describes the fusions.
#pragma once
#include <cassert>
#include <cstdint>
#include <cstring>
#include <utility>

struct abft_hip_ctx;

struct abft_hip_vector {
  abft_hip_ctx *ctx = nullptr;
  double *d = nullptr;
  int n = 0;
  bool owns = true;
  double *host = nullptr;  // pinned staging for map/unmap
  abft_hip_vector *root = nullptr;  // the allocation a view looks into (itself for an owner)
  bool exposed = false;             // root only: the raw device pointer was handed out
  int views = 0;                    // root only: live views into this allocation
};

// ---- predicates on handles and scalars ----

static inline bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

static inline bool disjoint(const abft_hip_vector *a, const abft_hip_vector *b) {
  return a->d + a->n <= b->d || b->d + b->n <= a->d;
}
static inline bool disjoint(const double *a, const double *b, int n) { return a + n <= b || b + n <= a; }

// a whole allocation nobody else can see into: its handle is the only way to its buffer, so a swap of the buffer
// behind the handle goes unseen
static inline bool plain_vector(const abft_hip_vector *v, int n) {
  return v && v->owns && v->root == v && !v->exposed && v->views == 0 && v->n == n && v->d;
}

// the loop's four vectors: whole allocations only the library can see into, of one length, none of them twice
static inline bool plain_loop_vectors(const abft_hip_vector *x, const abft_hip_vector *r, const abft_hip_vector *p,
                                      const abft_hip_vector *w) {
  if (!p || p->n <= 0) return false;
  const int n = p->n;
  return plain_vector(x, n) && plain_vector(r, n) && plain_vector(p, n) && plain_vector(w, n) && x != r && x != p &&
         x != w && r != p && r != w && p != w;
}

// ---- state, by owner ----

struct Shadow { double *buf = nullptr; int n = 0; };  // a context-owned buffer of n (+ 2) doubles (abft_hip.hip: shadow_ensure)

// cross-call fusion no. 1: the last spmv also produced vec . result (see FuseOut)
struct FusedProduct {
  bool valid = false, have_value = false;
  bool vecc = false;  // made by abft_hip_spmv_vecc: serves abft_hip_dot_vecc only (and a plain product a plain dot only)
  const double *x = nullptr, *y = nullptr;
  int n = 0;
  uint32_t seq = 0;
  double value = 0.0;
};

// cross-call fusion no. 2: calc_xr leaves x += alpha p to the calc_p that follows it (see kernels.hip, calc_r_kernel);
// anything else that comes first flushes it
struct DeferredUpdate {
  bool active = false, on_dev = false;  // on_dev: alpha was formed on the device (abft_hip_ctx::alpha_dev)
  double *x = nullptr;
  const double *p = nullptr;
  int n = 0;
  double alpha = 0.0;
};

// cross-call fusion no. 4: in the host-scalar loop the deferred x += alpha p is the one piece of work nothing waits
// for, so once the library has seen spmv(A, p, w) directly follow a calc_p that took a deferred update along
// (`armed`), that calc_p writes the new p into `shadow`, swaps it with p's buffer and leaves the update pending on
// the OLD p (`active`); the predicted spmv(A, p, w) -- streaming CSR, fused product -- applies it row by row under
// its own memory latency (spmv_csr_kernel<..., NUPD = 1>).  Anything else that comes first applies it with axpy_kernel
// (the prologue) and disarms.  Same bits either way; only when each x[i] is written changes.
struct PendingUpdate {
  bool armed = false, active = false;
  const abft_hip_vector *last_p = nullptr;  // set by the calc_p that consumed a deferred update on this p ...
  const abft_hip_vector *prev_p = nullptr;  // ... and handed to the entry point that follows it directly (the prologue)
  double *x = nullptr;                      // the pending update: x += alpha p_old over n elements
  const double *p_old = nullptr;
  double alpha = 0.0;
  int n = 0;
  const abft_hip_vector *ph = nullptr;      // the handle whose buffer was swapped
  // context-owned: where the next calc_p writes (the old p while pending).  Two slots by length, so that a caller who
  // alternates solves of two sizes does not free and allocate (both synchronise the device) at every switch
  Shadow shadow[2];
  int shadow_at = 0;                        // the slot used last
  long absorbed = 0, flushed = 0;
};

// cross-call fusion no. 6 (ABFT_HIP_LAZY_X=1|2|4): nobody reads x until the solve ends or a caller looks, yet the
// pending update costs its SpMV a read and a write of x every iteration.  With depth d > 1 the predicted SpMV that
// absorbs a pending update only QUEUES it -- the old p stays where it is, a spare buffer takes its place as the next
// calc_p's target -- until the queue and the pending update together make d: that SpMV applies all d in one pass
// (spmv_csr_kernel<..., NUPD = d>: x read once, written once, the d multiply-adds per element in arrival order).
// Four continuations of the predicted loop keep the queue: the eligible spmv(A, p, w), the dot served from its fused
// product, the calc_xr that defers its update onto the queue's x, and the calc_p that takes that update along.
// Everything else applies it first, in order, with one axpy_chain_kernel (the prologue).  Same bits either way.
// depth 1: no queue, nothing here is ever touched.
struct LazyUpdates {
  static constexpr int MAX_DEPTH = 4;
  struct Entry { double *p_old; double alpha; };
  int depth = 1;           // 1, 2 or 4; lowered for good when the spare buffers do not fit (abft_hip.hip: lazy_ring_ensure)
  double *x = nullptr;     // the queue's target: x += q[0].alpha * q[0].p_old, then q[1], ... over n elements
  int n = 0;
  int count = 0;
  Entry q[MAX_DEPTH] = {};
  // context-owned buffers of spare_n (+ 2) doubles nobody reads or writes: with the queued old p's and the one in
  // xpend.shadow they are the `depth` buffers that, with the one behind p's handle, make the ring of depth + 1
  double *spare[MAX_DEPTH - 1] = {};
  int nspare = 0, spare_n = 0;
  long bursts = 0, applied_in_bursts = 0, applied_by_flush = 0;
};
// updates to apply to x in one pass, oldest first
struct LazyBatch {
  double *x = nullptr;
  int n = 0, count = 0;
  LazyUpdates::Entry e[LazyUpdates::MAX_DEPTH] = {};
};

// The caller's iteration, as the library knows it: what the SpMV's fold, the speculation and the run-ahead all read.
struct CallerIteration {
  abft_hip_vector *x = nullptr, *r = nullptr, *p = nullptr, *w = nullptr;  // of the last calc_xr run as written
  bool have_rr = false;  // scal[2 * rr_at] holds the scalar last handed to the caller (r.r), whose value is rr_host
  int rr_at = 0;
  double rr_host = 0.0;
  double rr_prev = 0.0;  // the scalar handed back before rr_host: beta's denominator
  // device doubles: [0], [2] r.r (alternating), [4] p.w (abft_hip.hip, spmv_common: the fold's dev_out), each with its
  // event count behind
  double *scal = nullptr;
  // an r half in flight: where it writes and the sequence number of its r.r.  One buffer for both owners below: they
  // are never both on (loop_invariant)
  Shadow r_shadow;
  uint32_t seq_rr = 0;
};

// cross-call fusion no. 3 (opt-in: ABFT_HIP_SPECULATE=1): once the library has seen one iteration it enqueues, right
// behind the NEXT spmv(A, p, w) and its fold, the r half of that iteration with alpha = rr / p.w formed on the
// device, writing into iter.r_shadow, and -- once calc_xr has been taken over -- the x / p half (x in place, p into
// p_shadow).  When the caller's calc_xr / calc_p then arrive with the same vectors and bit-identical alpha / beta
// (the same IEEE quotients of the scalars it was handed), the shadows are swapped in -- no kernel is launched, the
// GPU never waited for the host; anything else drops the shadows and runs the call as written.  Same bits either way.
struct Speculation {
  bool enabled = false;
  bool learned = false;       // iter's x, r, p, w are the vectors of a complete iteration
  Shadow p_shadow;
  double rr_new_host = 0.0;   // the speculated r.r, handed back by the calc_xr that committed
  long commits = 0, drops = 0;
};

// cross-call fusion no. 5 (ABFT_HIP_AHEAD=0|1|2): the same idea with what x-in-SpMV left to do.  calc_p already
// writes out of place into xpend's buffer, so level 1 launches it right behind calc_r, BEFORE the host waits for
// r.r, with beta = rr_new / rr formed on the device (InFlight::AheadP); level 2 also launches calc_r behind the
// SpMV's fold with alpha = rr / p.w formed on the device, into iter.r_shadow, and the calc_p behind it
// (InFlight::AheadRP).  The caller's calc_xr / calc_p commit -- swap the buffers, launch nothing -- when they name the
// same vectors and alpha / beta are bit for bit the host's quotients of the scalars handed back (and no NaN: its
// payload is not the same on both sides); every other entry point drops through the prologue.  Armed by one complete
// iteration, run as written, whose alpha and beta were those quotients; a drop or an iteration with other scalars
// disarms.
struct RunAhead {
  int level = 0;
  bool armed = false;
  bool alpha_ok = false;  // the calc_xr just run was handed rr / p.w on plain vectors (cleared by any entry point but calc_p)
  int slot = 0;           // xpend.shadow[slot]: where the calc_p in flight writes
  long commit_p = 0, commit_r = 0, drops = 0;
  // ABFT_HIP_DEFER_FINISH: a reduction whose consumer kernel is launched behind it in the same call -- calc_r before
  // the calc_p run ahead, at level 2 also the fused p.w's fold before calc_r -- leaves its finish (the fold of the
  // block partials, the published scalar) to the head of that consumer.  The same launches carrying the same bits:
  // no state of its own, nothing to commit or drop.  Off wherever the run-ahead is (loop_settle_switches).
  bool defer_finish = false;
};

// what has been launched ahead of the call that will ask for it
enum class InFlight {
  None,
  SpecR,     // speculation: the r half (its x / p half follows when calc_xr has been taken over)
  SpecXP,    // speculation: r committed, the x / p half pending
  AheadP,    // run-ahead: calc_p
  AheadRP,   // run-ahead: calc_r and the calc_p behind it
};

struct LoopState {
  bool capturing = false;     // between abft_hip_graph_begin and _end
  bool fuse_enabled = true;   // ABFT_HIP_FUSE_DOT
  bool defer_enabled = true;  // ABFT_HIP_FUSE_X
  // ABFT_HIP_X_IN_SPMV=0 / =1; by default on the modes of ABFT_X_IN_SPMV_MODES; off without the deferred update or the
  // fused product, with the speculation, and from the first graph capture on (a captured launch holds p's buffer by address)
  bool xin_enabled = true;
  unsigned xin_modes = 0;     // bit m: armed on matrices of ECC mode m (ABFT_HIP_X_IN_SPMV=1: every mode)
  FusedProduct fused;
  DeferredUpdate defer;
  PendingUpdate xpend;
  LazyUpdates lazy;
  CallerIteration iter;
  Speculation spec;
  RunAhead ahead;
  InFlight flight = InFlight::None;
};

// What abft_hip_init settles, once: the run-ahead writes where xpend's calc_p writes and commits by xpend's swap, and
// x-in-SpMV is off with the speculation.  So at most one of the two can ever have anything in flight.
static inline void loop_settle_switches(LoopState &L) {
  L.xin_enabled = L.xin_enabled && L.defer_enabled && L.fuse_enabled && !L.spec.enabled;
  if (!L.xin_enabled) L.ahead.level = 0;
  if (L.ahead.level == 0) L.ahead.defer_finish = false;
  // the queue hangs off x-in-SpMV's pending update: no such path, no queue
  if (!L.xin_enabled || (L.lazy.depth != 2 && L.lazy.depth != 4)) L.lazy.depth = 1;
}
static inline bool loop_invariant(const LoopState &L) {
  return (!L.spec.enabled || !L.xin_enabled) && (L.xin_enabled || L.ahead.level == 0);
}
static inline void set_in_flight(LoopState &L, InFlight f) {
  assert(loop_invariant(L));
  assert(f == InFlight::None || (f == InFlight::SpecR || f == InFlight::SpecXP ? L.spec.enabled : L.ahead.level > 0));
  L.flight = f;
}

// ---- the device scalars ----

struct ScalTriple { double *rr, *rr_new, *pw; };  // r.r as the caller holds it, where the next r.r goes, p.w
static inline ScalTriple scal_triple(const CallerIteration &I) {
  return {I.scal + 2 * I.rr_at, I.scal + 2 * (1 - I.rr_at), I.scal + 4};
}
// the slot of a reduction run as written whose result the caller will hold as r.r (never the one it holds now) ...
static inline int rr_next_at(const CallerIteration &I) { return I.have_rr ? 1 - I.rr_at : 0; }
// ... and that result handed back
static inline void rr_handed(CallerIteration &I, int at, double value) {
  I.have_rr = true; I.rr_at = at; I.rr_host = value;
}

// ---- drop, forget ----

// What is in flight is void: its shadow buffers are never looked at again.  A run-ahead leaves r and p untouched and
// the scalars as the caller holds them; a speculation whose r half was committed keeps the committed r and the x
// already updated in place -- calc_xr is done; what the caller holds as r.r is the speculated one.
static inline void drop_in_flight(LoopState &L) {
  L.ahead.alpha_ok = false;
  switch (L.flight) {
    case InFlight::None: return;
    case InFlight::AheadP:
    case InFlight::AheadRP:
      L.ahead.drops++;
      L.ahead.armed = false;
      break;
    case InFlight::SpecXP:
      L.iter.rr_at = 1 - L.iter.rr_at;
      L.iter.rr_host = L.spec.rr_new_host;
      [[fallthrough]];
    case InFlight::SpecR:
      L.spec.drops++;
      break;
  }
  set_in_flight(L, InFlight::None);
}

// ... and nothing is known about the caller's iteration any more (the learned iteration names vectors by handle)
static inline void forget_iteration(LoopState &L) {
  drop_in_flight(L);
  L.spec.learned = false;
  L.ahead.armed = false;
  L.iter.have_rr = false;
  L.iter.x = L.iter.r = L.iter.p = L.iter.w = nullptr;
}

static inline void forget_fused(LoopState &L) { L.fused.valid = false; }
// a reduction is about to take a pinned slot: a fused product nobody has read yet may lose its own
static inline void fused_slot_reused(LoopState &L) {
  if (!L.fused.have_value) L.fused.valid = false;
}

// ---- the prologue of every entry point: its state part ----

// What an entry point keeps of the state above.  Without a flag: what is in flight is dropped, the update pending on
// the old p and the deferred one are applied (abft_hip.hip: enter), the fused product and the learned iteration stay.
enum : unsigned {
  KEEP_DEFERRED = 1u,  // touches no vector, or is the calc_p that can take x += alpha p along (keeps the pending one too)
  KEEP_FLIGHT = 2u,    // one of the continuations what is in flight waits for -- dot(p, w), calc_xr, calc_p: decides itself
  KEEP_PENDING = 4u,   // the SpMV that may absorb the update pending on the old p: decides itself
  FORGET_FUSED = 8u,   // writes a vector the fused product may name
  FORGET_ITER = 16u,   // works on vectors the learned iteration may name, in a way the loop's bookkeeping does not follow
  KEEP_LAZY = 32u,     // one of the four continuations that keep the queue of x updates (LazyUpdates): decides itself
};

static inline void prologue_begin(LoopState &L, unsigned keep) {
  L.xpend.prev_p = L.xpend.last_p;
  L.xpend.last_p = nullptr;
  if (!(keep & KEEP_FLIGHT)) drop_in_flight(L);
}
static inline bool prologue_flushes_pending(unsigned keep) { return !(keep & (KEEP_DEFERRED | KEEP_PENDING)); }
static inline bool prologue_flushes_deferred(unsigned keep) { return !(keep & KEEP_DEFERRED); }
static inline bool prologue_flushes_lazy(unsigned keep) { return !(keep & KEEP_LAZY); }
static inline void prologue_end(LoopState &L, unsigned keep) {
  if (keep & FORGET_FUSED) forget_fused(L);
  if (keep & FORGET_ITER) forget_iteration(L);
}

// the pending x += alpha p_old is due on its own (something other than the predicted SpMV came first): true -> the
// caller launches x += alpha p_old over n from the fields of xpend
static inline bool pending_flush_due(LoopState &L) {
  auto &X = L.xpend;
  if (!X.active) return false;
  X.active = false;
  X.armed = false;
  X.flushed++;
  return true;
}
static inline bool deferred_flush_due(LoopState &L) {
  if (!L.defer.active) return false;
  L.defer.active = false;
  return true;
}

// ---- fusion no. 1: the fused product ----

static inline bool fused_serves_dot(const LoopState &L, const abft_hip_vector *a, const abft_hip_vector *b, bool vecc) {
  const auto &F = L.fused;
  return F.valid && F.vecc == vecc && a->n == F.n && ((a->d == F.x && b->d == F.y) || (a->d == F.y && b->d == F.x));
}
static inline void fused_value_read(LoopState &L, double value) {
  L.fused.value = value;
  L.fused.have_value = true;
}
static inline void fused_made(LoopState &L, bool vecc, const abft_hip_vector *vec, const abft_hip_vector *result,
                              uint32_t seq) {
  auto &F = L.fused;
  F.valid = true;
  F.have_value = false;
  F.vecc = vecc;
  F.x = vec->d;
  F.y = result->d;
  F.n = vec->n;
  F.seq = seq;
}

// ---- fusion no. 2: the deferred update ----

// x += alpha p can wait for the calc_p that reads the same p next (one pass over p less per iteration) when nobody can
// look at x in between: x is not aliased by any other operand and its raw pointer has never been handed out
static inline bool can_defer_x(const LoopState &L, const abft_hip_vector *x, const abft_hip_vector *r,
                               const abft_hip_vector *p, const abft_hip_vector *w) {
  return L.defer_enabled && x->n > 0 && !(x->root ? x->root : x)->exposed && disjoint(x, r) && disjoint(x, p) &&
         disjoint(x, w) && disjoint(r, p);
}
static inline void arm_deferred(LoopState &L, const abft_hip_vector *x, const abft_hip_vector *p, double alpha,
                                bool on_dev) {
  auto &D = L.defer;
  D.active = true;
  D.on_dev = on_dev;
  D.x = x->d; D.p = p->d; D.n = x->n; D.alpha = alpha;
}
// is calc_p(p, r) the call the deferred update waits for?
static inline bool deferred_rides_with(const LoopState &L, const abft_hip_vector *p, const abft_hip_vector *r) {
  const auto &D = L.defer;
  return D.active && D.p == p->d && D.n == p->n && (D.x + D.n <= r->d || r->d + r->n <= D.x);
}

// ---- fusion no. 4: the update pending on the old p ----

// may this calc_p(p, r) write its p out of place and leave the deferred update pending?  (the shadow permitting)
static inline bool pending_can_take(const LoopState &L, const abft_hip_vector *p, const abft_hip_vector *r) {
  const auto &X = L.xpend;
  if (!L.xin_enabled || !X.armed || X.active || L.defer.on_dev || L.capturing) return false;
  return plain_vector(p, p->n) && disjoint(p, r);
}
// the same question for a calc_p launched ahead (the caller has checked the vectors)
static inline bool pending_can_run_ahead(const LoopState &L) {
  const auto &X = L.xpend;
  return L.xin_enabled && X.armed && !X.active && !L.capturing;
}
// the slot of xpend.shadow for a new p of n entries: the one of that length, else the one not used last (abft_hip.hip,
// xpend_buffer, allocates it for this length)
static inline int pending_shadow_slot(const PendingUpdate &X, int n) {
  if (X.shadow[0].buf && X.shadow[0].n == n) return 0;
  if (X.shadow[1].buf && X.shadow[1].n == n) return 1;
  return X.shadow[X.shadow_at].buf ? 1 - X.shadow_at : X.shadow_at;
}
// The new p is in xpend.shadow[at] (launched as written, or ahead): p adopts it by swap, and the deferred
// x += alpha p stays pending on the old one.
static inline void adopt_p_leave_pending(LoopState &L, abft_hip_vector *p, int at) {
  auto &X = L.xpend;
  L.defer.active = false;
  std::swap(p->d, X.shadow[at].buf);
  X.active = true;
  X.x = L.defer.x; X.p_old = X.shadow[at].buf; X.alpha = L.defer.alpha; X.n = p->n; X.ph = p;
}
// the switches' part of the question whether an SpMV on a matrix of this ECC mode could apply a pending update ...
static inline bool pending_path_on(const LoopState &L, unsigned mode) {
  return L.xin_enabled && (L.xin_modes >> mode & 1u) && !L.capturing && L.fuse_enabled;
}
// ... and whether this one does.  `eligible`: the path is on and the call is abft_hip_spmv(A, p, w) on the streaming CSR
// layout, whole, with the fused product (abft_hip.hip, spmv_can_absorb: the matrix is there).
// Also where the prediction is armed: such a call on a plain p directly after the calc_p that took a deferred update
// on that p along.
static inline bool pending_absorbed_by(LoopState &L, bool eligible, const abft_hip_vector *vec,
                                       const abft_hip_vector *result) {
  auto &X = L.xpend;
  const abft_hip_vector *after_calc_p = X.prev_p;
  X.prev_p = nullptr;
  if (!eligible) return false;
  if (!X.active) {
    if (after_calc_p == vec && plain_vector(vec, vec->n)) X.armed = true;
    return false;
  }
  return X.ph == vec && X.n == vec->n && disjoint(X.x, result->d, X.n) && disjoint(X.p_old, result->d, X.n);
}
static inline void pending_absorbed(LoopState &L) {  // applied exactly once, whatever the launch reports about the matrix
  L.xpend.active = false;
  L.xpend.absorbed++;
}

// ---- fusion no. 6: the queue of x updates ----

// Everything queued is due on its own (something other than the four keeping continuations came): true -> the caller
// applies `out` with one launch.  The old p's go back to the spares behind that launch, in stream order.
static inline bool lazy_flush_due(LoopState &L, LazyBatch &out) {
  auto &Z = L.lazy;
  if (Z.count == 0) return false;
  out.x = Z.x; out.n = Z.n; out.count = Z.count;
  for (int k = 0; k < Z.count; k++) {
    out.e[k] = Z.q[k];
    assert(Z.nspare < LazyUpdates::MAX_DEPTH - 1);
    Z.spare[Z.nspare++] = Z.q[k].p_old;
  }
  Z.applied_by_flush += Z.count;
  Z.count = 0;
  return true;
}
// Take or apply, once pending_absorbed_by has said "absorb".  First: a pending update on another x or length than the
// queue's does not join it -- the caller flushes the queue ...
static inline bool lazy_queue_mismatch(const LoopState &L) {
  const auto &Z = L.lazy;
  return Z.count > 0 && (Z.x != L.xpend.x || Z.n != L.xpend.n);
}
// ... and, the queue empty, has the spares of this length ready before it asks (false: lazy_ring_ensure is due)
static inline bool lazy_ring_ready(const LoopState &L) {
  const auto &Z = L.lazy;
  return Z.depth <= 1 || Z.count > 0 || (Z.spare_n == L.xpend.n && Z.nspare == Z.depth - 1);
}
enum class LazyStep {
  ApplyOne,  // depth 1: this SpMV applies the pending update, as ever (pending_absorbed)
  Queue,     // the pending update joins the queue, this SpMV applies nothing (lazy_queue_pending)
  Burst,     // the queue and the pending update make `depth`: this SpMV applies them all (lazy_burst)
};
static inline LazyStep lazy_step(const LoopState &L) {
  const auto &Z = L.lazy;
  assert(L.xpend.active && !lazy_queue_mismatch(L) && lazy_ring_ready(L));
  if (Z.depth <= 1) return LazyStep::ApplyOne;
  if (Z.count + 1 >= Z.depth) return LazyStep::Burst;
  assert(Z.nspare > 0);
  return LazyStep::Queue;
}
// The pending update is the queue's youngest entry; its SpMV has taken it over (`absorbed`).  The old p stays put: a
// spare takes its place in xpend.shadow, where the next calc_p -- as written or run ahead -- writes.
static inline void lazy_queue_pending(LoopState &L) {
  auto &Z = L.lazy;
  auto &X = L.xpend;
  double *old = const_cast<double *>(X.p_old);
  Z.x = X.x; Z.n = X.n;
  Z.q[Z.count++] = {old, X.alpha};
  for (auto &s : X.shadow)
    if (s.buf == old) s.buf = Z.spare[--Z.nspare];
  pending_absorbed(L);
}
// The queue, then the pending update: what this SpMV applies.  The queued old p's are spares again behind it.
static inline LazyBatch lazy_burst(LoopState &L) {
  auto &Z = L.lazy;
  const auto &X = L.xpend;
  LazyBatch b;
  b.x = X.x; b.n = X.n;
  for (int k = 0; k < Z.count; k++) {
    b.e[b.count++] = Z.q[k];
    Z.spare[Z.nspare++] = Z.q[k].p_old;
  }
  b.e[b.count++] = {const_cast<double *>(X.p_old), X.alpha};
  Z.count = 0;
  Z.bursts++;
  Z.applied_in_bursts += b.count;
  pending_absorbed(L);
  return b;
}
// calc_xr(x, r, p, w) keeps the queue when it defers its own update (can_defer_x) onto the queue's x
static inline bool lazy_kept_by_calc_xr(const LoopState &L, const abft_hip_vector *x, const abft_hip_vector *r,
                                        const abft_hip_vector *p, const abft_hip_vector *w) {
  const auto &Z = L.lazy;
  if (Z.count == 0) return true;
  return x && r && p && w && x->d == Z.x && x->n == Z.n && can_defer_x(L, x, r, p, w);
}

// ---- the two quotients ----

// Was alpha the quotient of the two scalars the caller was handed -- r.r and the fused p.w of spmv(A, p, w)?
// (`no_nan`: the run-ahead's form; a NaN's payload is not the same on the host and on the device)
static inline bool alpha_was_rr_over_pw(const LoopState &L, double alpha, bool no_nan) {
  return (!no_nan || alpha == alpha) && same_bits(alpha, L.iter.rr_host / L.fused.value);
}
// ... and beta the quotient of the last two residuals handed back?
static inline bool beta_was_quotient(double beta, double rr_new, double rr, bool no_nan) {
  return (!no_nan || beta == beta) && same_bits(beta, rr_new / rr);
}

// ---- behind spmv(A, p, w) and its fold ----

// fusion no. 3: launch the learned iteration's r half?
static inline bool spec_wants_r(const LoopState &L, const abft_hip_vector *vec, const abft_hip_vector *result) {
  const auto &I = L.iter;
  if (!L.spec.enabled || !L.spec.learned || !I.have_rr || L.flight != InFlight::None || L.defer.active || L.capturing)
    return false;
  if (vec != I.p || result != I.w) return false;
  const int n = vec->n;
  return n > 0 && plain_vector(I.x, n) && plain_vector(I.r, n) && plain_vector(I.p, n) && plain_vector(I.w, n);
}
// fusion no. 5, level 2: launch calc_r and calc_p?  (`eligible`: as for pending_absorbed_by)
static inline bool ahead_wants_rp(const LoopState &L, bool eligible, const abft_hip_vector *vec,
                                  const abft_hip_vector *result) {
  const auto &I = L.iter;
  if (!eligible || L.ahead.level < 2 || !L.ahead.armed || L.flight != InFlight::None || !I.have_rr || L.defer.active ||
      L.capturing)
    return false;
  if (vec != I.p || result != I.w || !plain_loop_vectors(I.x, I.r, I.p, I.w)) return false;
  return L.xin_enabled && L.xpend.armed && !L.xpend.active;
}
// the r half is in flight, its r.r on the way to pinned slot seq
static inline void r_half_launched(LoopState &L, InFlight f, uint32_t seq) {
  L.iter.seq_rr = seq;
  set_in_flight(L, f);
}

// ---- abft_hip_calc_xr ----

enum class XrOutcome { AsWritten, CommitAhead, TrySpec };
struct XrCall {
  XrOutcome outcome;
  bool alpha_ok;  // alpha was rr / p.w, no NaN, on plain vectors (only ever true with the run-ahead on)
  double rr_old;  // the r.r the caller held when it called
};

// Which of the three is this call?  Whatever is in flight and does not match it is dropped here.  TrySpec: the vectors
// are the speculated ones; whether alpha matches is known once the fused p.w has been read (spec_r_matches_alpha).
static inline XrCall classify_calc_xr(LoopState &L, const abft_hip_vector *x, const abft_hip_vector *r,
                                      const abft_hip_vector *p, const abft_hip_vector *w, double alpha) {
  const auto &I = L.iter;
  const auto &F = L.fused;
  XrCall c{XrOutcome::AsWritten, false, I.rr_host};
  c.alpha_ok = L.ahead.level && I.have_rr && F.valid && F.have_value && !F.vecc && p && w && F.x == p->d && F.y == w->d &&
               alpha_was_rr_over_pw(L, alpha, true) && plain_loop_vectors(x, r, p, w);
  const bool same_vectors = x == I.x && r == I.r && p == I.p && w == I.w;
  if (L.flight == InFlight::AheadRP && c.alpha_ok && same_vectors) c.outcome = XrOutcome::CommitAhead;
  // (a view made since the launch -- abft_hip_vector_view drops nothing -- looks into r's buffer: no swap behind it)
  else if (L.flight == InFlight::SpecR && same_vectors && F.valid && plain_vector(r, r->n)) c.outcome = XrOutcome::TrySpec;
  else drop_in_flight(L);
  return c;
}

// The calc_r that ran ahead is this very call: r's buffer and the shadow change places, x += alpha p is left to the
// calc_p as a calc_xr run as written leaves it, and the calc_p behind it stays in flight.  rr_new: read from the slot.
static inline void commit_ahead_r(LoopState &L, const XrCall &c, abft_hip_vector *x, abft_hip_vector *r,
                                  const abft_hip_vector *p, double alpha, double rr_new) {
  auto &I = L.iter;
  std::swap(r->d, I.r_shadow.buf);
  forget_fused(L);
  arm_deferred(L, x, p, alpha, false);
  I.rr_prev = c.rr_old;
  I.rr_at = 1 - I.rr_at;
  I.rr_host = rr_new;
  set_in_flight(L, InFlight::AheadP);
  L.ahead.alpha_ok = true;
  L.ahead.commit_r++;
}

// The speculated r half is this very call (the caller has enqueued the x / p half and read the speculated r.r): r is
// now what calc_r left in the shadow; its old buffer is the next shadow.
static inline void commit_spec_r(LoopState &L, abft_hip_vector *r, double rr_new) {
  std::swap(r->d, L.iter.r_shadow.buf);
  forget_fused(L);
  set_in_flight(L, InFlight::SpecXP);
  L.spec.rr_new_host = rr_new;
}

// calc_xr run as written: is the calc_p that will follow launched behind it (level 1)?  Also where an alpha that was
// not the quotient disarms.  Asked after the launch (the deferred update it left is part of the answer).
static inline bool ahead_wants_p(LoopState &L, const XrCall &c, const abft_hip_vector *p) {
  if (!c.alpha_ok) L.ahead.armed = false;
  return c.alpha_ok && L.ahead.armed && L.defer.active && !L.defer.on_dev && L.defer.p == p->d && pending_can_run_ahead(L);
}
// The same question asked BEFORE the launch, without the side effect: will ahead_wants_p say yes once this calc_xr has
// gone out?  (can_defer_x: the launch then is calc_r and leaves x += alpha p deferred on this p, with alpha on the
// host.)  Then calc_r may leave the finish of r.r to that calc_p -- the shadow for the new p permitting, which the
// caller secures before it launches either.
static inline bool xr_can_defer_finish(const LoopState &L, const XrCall &c, const abft_hip_vector *x,
                                       const abft_hip_vector *r, const abft_hip_vector *p, const abft_hip_vector *w) {
  return L.ahead.defer_finish && c.alpha_ok && L.ahead.armed && can_defer_x(L, x, r, p, w) && pending_can_run_ahead(L);
}
// ... and what it leaves behind once its r.r (slot `at` of scal) has been handed back: what the run-ahead and a
// speculation need to know about this iteration
static inline void calc_xr_ran(LoopState &L, const XrCall &c, bool p_ahead, int at, double rr_new, abft_hip_vector *x,
                               abft_hip_vector *r, const abft_hip_vector *p, const abft_hip_vector *w) {
  auto &I = L.iter;
  if (p_ahead) set_in_flight(L, InFlight::AheadP);
  L.ahead.alpha_ok = c.alpha_ok;
  I.rr_prev = c.rr_old;
  rr_handed(I, at, rr_new);
  I.x = x; I.r = r; I.p = const_cast<abft_hip_vector *>(p); I.w = const_cast<abft_hip_vector *>(w);
  L.spec.learned = false;  // ... until the calc_p that completes it
}

// ---- abft_hip_calc_p ----

enum class POutcome { AsWritten, CommitAhead, CommitSpec };
struct PCall {
  POutcome outcome;
  bool beta_ok;  // beta was rr_new / rr behind a calc_xr whose alpha was its quotient, no NaN, on plain vectors
};

static inline PCall classify_calc_p(LoopState &L, const abft_hip_vector *p, const abft_hip_vector *r, double beta) {
  const auto &I = L.iter;
  PCall c{POutcome::AsWritten, false};
  c.beta_ok = L.ahead.alpha_ok && p == I.p && r == I.r && beta_was_quotient(beta, I.rr_host, I.rr_prev, true) &&
              plain_loop_vectors(I.x, I.r, I.p, I.w);
  if (L.flight == InFlight::AheadP && c.beta_ok && L.defer.active && !L.defer.on_dev && L.defer.p == p->d &&
      L.defer.n == p->n && !L.xpend.active)
    c.outcome = POutcome::CommitAhead;
  // (p must still be a vector only the library sees into: a view of it may have been made since calc_xr)
  else if (L.flight == InFlight::SpecXP && p == I.p && r == I.r &&
           beta_was_quotient(beta, L.spec.rr_new_host, I.rr_host, false) && !L.defer.active && plain_vector(p, p->n))
    c.outcome = POutcome::CommitSpec;
  else
    drop_in_flight(L);
  return c;
}

// the calc_p that ran ahead is this very call: what a calc_p that takes the pending path does behind its launch, and no launch
static inline void commit_ahead_p(LoopState &L, abft_hip_vector *p) {
  adopt_p_leave_pending(L, p, L.ahead.slot);
  L.xpend.last_p = p;
  forget_fused(L);
  set_in_flight(L, InFlight::None);
  L.ahead.commit_p++;
}

// the speculated x / p half is this very call: the speculated r.r is the residual the caller now holds
static inline void commit_spec_p(LoopState &L, abft_hip_vector *p) {
  std::swap(p->d, L.spec.p_shadow.buf);
  forget_fused(L);
  set_in_flight(L, InFlight::None);
  L.iter.rr_at = 1 - L.iter.rr_at;
  L.iter.rr_host = L.spec.rr_new_host;
  L.spec.commits++;
}

// calc_p run as written, before its launch: does calc_p(p, r) right behind calc_xr(x, r, p, w) complete an iteration
// of the CG loop? ...
static inline bool completes_iteration(const LoopState &L, const abft_hip_vector *p, const abft_hip_vector *r) {
  const auto &I = L.iter;
  return I.have_rr && !L.spec.learned && I.p == p && I.r == r && I.x && I.w;
}
// ... and after it: one complete iteration on the two quotients arms the run-ahead, any other disarms
static inline void calc_p_ran(LoopState &L, const PCall &c, bool completes, const abft_hip_vector *p,
                              const abft_hip_vector *r) {
  L.ahead.armed = L.ahead.level && c.beta_ok;
  L.spec.learned = completes || (L.spec.learned && L.iter.p == p && L.iter.r == r);
}
