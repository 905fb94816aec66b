// lazy_x_play.cpp -- the queue of x updates (abft_sparse_cg_amd/csrc/loop_state.h, LazyUpdates) played without a GPU:
// this program stands where abft_hip.hip stands, as tests/host/loop_state_play.cpp does for the older fusions, and
// holds every decision against a plain model: a first-in first-out list of the updates x += alpha p that calc_xr has
// left behind, each naming its x, its alpha and the buffer its p lives in.  tests/test_lazy_x_host.py builds it with
// -fsanitize=address,undefined and feeds it scripts on stdin, any number of them:
//
//   begin XIN AHEAD SPEC DEPTH   the switches as abft_hip_init reads them (loop_state_play.cpp) and ABFT_HIP_LAZY_X
//   dot A B BITS                 abft_hip_dot(A, B)
//   spmv                         abft_hip_spmv(A, p, w), the eligible one
//   spmv_q                       abft_hip_spmv(A, q, w): any other SpMV
//   xr ALPHA RR_NEW              abft_hip_calc_xr(x, r, p, w, ALPHA)
//   xr_q ALPHA RR_NEW            abft_hip_calc_xr(q, r, p, w, ALPHA): a calc_xr on another x
//   p BETA                       abft_hip_calc_p(p, r, BETA)
//   other                        an entry point with no flags (abft_hip_synchronize, a download, graph_begin ...)
//   nomem K                      from now on only K more spare buffers can be allocated
//   show / end                   print committed_p committed_r dropped absorbed flushed spec_commits spec_drops in_flight
//                                bursts applied_in_bursts applied_by_flush depth; `end` first shuts the context down
// A broken rule ends the program with a message and status 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <set>
#include <string>

#include "loop_state.h"

#ifndef ABFT_AHEAD_DEFAULT
#error "build with -DABFT_AHEAD_DEFAULT=... -DABFT_X_IN_SPMV_MODES=... as abft_internal.h has them"
#endif

static const int N = 8;
static double arena[24][N + 2];  // x, r, p, w, q, then the context's buffers as they are asked for

struct Update { const double *x; double alpha; const double *buf; };

struct Ctx : LoopState {
  abft_hip_vector v[5];
  int next_buf = 5;
  uint32_t seq = 0;
  int configured = 1;
  int spares_left = 1 << 20;
  std::deque<Update> owed;           // the model: updates left behind and not yet applied, oldest first
  long applied = 0, arrived = 0;
  const double *ahead_target = nullptr;  // where a calc_p run ahead writes
  abft_hip_vector *vec(char c) { return &v[c == 'x' ? 0 : c == 'r' ? 1 : c == 'p' ? 2 : c == 'w' ? 3 : 4]; }
};

[[noreturn]] static void broken(const char *what) {
  fprintf(stderr, "lazy_x_play: %s\n", what);
  exit(3);
}

static double from_bits(const char *s) {
  const unsigned long long u = strtoull(s, nullptr, 16);
  double d;
  memcpy(&d, &u, sizeof(d));
  return d;
}

// ---- the model ----

static void arrives(Ctx &C, const double *x, double alpha, const double *buf) {
  C.owed.push_back({x, alpha, buf});
  C.arrived++;
}
// exactly once and in arrival order: whatever is applied is the oldest update owed
static void applies(Ctx &C, const double *x, double alpha, const double *buf) {
  if (C.owed.empty()) broken("an update applied that nobody owes (twice?)");
  const Update u = C.owed.front();
  C.owed.pop_front();
  if (u.x != x || !same_bits(u.alpha, alpha) || u.buf != buf) broken("an update applied out of arrival order, or not as it arrived");
  C.applied++;
}
static void applies(Ctx &C, const LazyBatch &b) {
  if (b.count < 1 || b.count > LazyUpdates::MAX_DEPTH) broken("a batch of no or too many updates");
  for (int k = 0; k < b.count; k++) applies(C, b.x, b.e[k].alpha, b.e[k].p_old);
}
// a calc_p is told to write `target`: never a buffer an update still owed reads, never p's own
static void writes_p(Ctx &C, const double *target) {
  if (!target) broken("calc_p told to write nowhere");
  if (target == C.vec('p')->d) broken("calc_p told to write p's own buffer out of place");
  for (const Update &u : C.owed)
    if (u.buf == target) broken("calc_p told to write a buffer a queued update still reads");
  for (int k = 0; k < C.lazy.nspare; k++)
    if (C.lazy.spare[k] == target) broken("calc_p told to write a spare");
}
// p's buffer, xpend's, the queued and the spare ones of p's length: all different, at most depth + 1 of them
static void ring_holds(const Ctx &C) {
  std::set<const double *> live;
  size_t want = 1;
  live.insert(C.v[2].d);
  for (const Shadow &s : C.xpend.shadow)
    if (s.buf) { live.insert(s.buf); want++; }
  for (int k = 0; k < C.lazy.count; k++) { live.insert(C.lazy.q[k].p_old); want++; }
  for (int k = 0; k < C.lazy.nspare; k++) { live.insert(C.lazy.spare[k]); want++; }
  if (live.size() != want) broken("a buffer in two places of the ring");
  if ((int)live.size() > C.configured + 1) broken("more than depth + 1 buffers live");
  if (C.lazy.count > 0 && C.lazy.count >= C.lazy.depth) broken("the queue holds a full burst");
  if (C.lazy.depth == 1 && (C.lazy.count || C.lazy.nspare || C.lazy.bursts || C.lazy.applied_by_flush))
    broken("depth 1 touched the queue");
}

// ---- what abft_hip.hip does around the decisions ----

static void shadow_ensure(Ctx &C, Shadow &s) {
  if (s.buf && s.n == N) return;
  if (C.next_buf >= 24) abort();
  s.buf = arena[C.next_buf++];
  s.n = N;
}
static int xpend_buffer(Ctx &C) {
  const int at = pending_shadow_slot(C.xpend, N);
  shadow_ensure(C, C.xpend.shadow[at]);
  C.xpend.shadow_at = at;
  return at;
}
static void lazy_ring_ensure(Ctx &C) {
  auto &Z = C.lazy;
  if (lazy_ring_ready(C)) return;
  Z.nspare = 0;  // (one length only here: nothing to free)
  Z.spare_n = C.xpend.n;
  while (Z.nspare < Z.depth - 1) {
    if (C.spares_left > 0) {
      if (C.next_buf >= 24) abort();
      C.spares_left--;
      Z.spare[Z.nspare++] = arena[C.next_buf++];
      continue;
    }
    Z.depth = Z.nspare >= 1 ? 2 : 1;
    while (Z.nspare > Z.depth - 1) --Z.nspare;
  }
}

static void flush_lazy(Ctx &C) {
  LazyBatch b;
  if (lazy_flush_due(C, b)) applies(C, b);
}
static void flush_xpend(Ctx &C) {
  if (!C.xpend.active) return;
  flush_lazy(C);
  if (pending_flush_due(C)) applies(C, C.xpend.x, C.xpend.alpha, C.xpend.p_old);
}
static void flush_deferred(Ctx &C) {
  if (!C.defer.active) return;
  flush_lazy(C);
  if (deferred_flush_due(C)) applies(C, C.defer.x, C.defer.alpha, C.defer.p);
}

static void enter(Ctx &C, unsigned keep) {
  prologue_begin(C, keep);
  if (prologue_flushes_lazy(keep)) flush_lazy(C);
  if (prologue_flushes_pending(keep)) flush_xpend(C);
  if (prologue_flushes_deferred(keep)) flush_deferred(C);
  prologue_end(C, keep);
  if (prologue_flushes_lazy(keep) && C.lazy.count) broken("a non-keeping entry left the queue filled");
}

static void play_dot(Ctx &C, const abft_hip_vector *a, const abft_hip_vector *b, double published) {
  enter(C, KEEP_FLIGHT | KEEP_LAZY);
  if (fused_serves_dot(C, a, b, false)) {
    if (!C.fused.have_value) fused_value_read(C, published);
    return;
  }
  drop_in_flight(C);
  flush_lazy(C);
  fused_slot_reused(C);
  rr_handed(C.iter, rr_next_at(C.iter), published);
  ++C.seq;
  if (C.lazy.count) broken("a dot run as written left the queue filled");
}

static void play_spmv(Ctx &C, char which) {
  const abft_hip_vector *vec = C.vec(which), *result = C.vec('w');
  enter(C, KEEP_PENDING | KEEP_LAZY);
  const bool eligible = pending_path_on(C, 0u);
  const bool absorb = pending_absorbed_by(C, eligible, vec, result);
  if (!absorb) {
    flush_lazy(C);
    flush_xpend(C);
    if (C.lazy.count) broken("another SpMV left the queue filled");
  }
  forget_fused(C);
  if (absorb) {
    if (lazy_queue_mismatch(C)) flush_lazy(C);
    lazy_ring_ensure(C);
    switch (lazy_step(C)) {
      case LazyStep::ApplyOne:
        if (C.lazy.count) broken("one update applied past a filled queue");
        applies(C, C.xpend.x, C.xpend.alpha, C.xpend.p_old);
        pending_absorbed(C);
        break;
      case LazyStep::Queue:
        if (C.lazy.depth == 1) broken("depth 1 queued");
        lazy_queue_pending(C);
        break;
      case LazyStep::Burst: {
        const LazyBatch b = lazy_burst(C);
        if (b.count != C.lazy.depth) broken("a burst of other than depth updates");
        applies(C, b);
        break;
      }
    }
    if (C.xpend.active) broken("the absorbing SpMV left the update pending");
  }
  if (!C.fuse_enabled) return;
  fused_made(C, false, vec, result, ++C.seq);
  if (spec_wants_r(C, vec, result)) {
    shadow_ensure(C, C.iter.r_shadow);
    shadow_ensure(C, C.spec.p_shadow);
    r_half_launched(C, InFlight::SpecR, ++C.seq);
  }
  if (ahead_wants_rp(C, eligible, vec, result)) {
    shadow_ensure(C, C.iter.r_shadow);
    (void)xpend_buffer(C);
    r_half_launched(C, InFlight::AheadRP, ++C.seq);
    C.ahead.slot = xpend_buffer(C);
    C.ahead_target = C.xpend.shadow[C.ahead.slot].buf;
    writes_p(C, C.ahead_target);
  }
}

static void play_calc_xr(Ctx &C, char which, double alpha, double rr_new) {
  abft_hip_vector *x = C.vec(which), *r = C.vec('r'), *p = C.vec('p'), *w = C.vec('w');
  enter(C, KEEP_FLIGHT | KEEP_LAZY);
  if (!lazy_kept_by_calc_xr(C, x, r, p, w)) flush_lazy(C);
  if (C.lazy.count && C.lazy.x != x->d) broken("a calc_xr on another x left the queue filled");
  const XrCall c = classify_calc_xr(C, x, r, p, w, alpha);
  if (c.outcome == XrOutcome::CommitAhead) {
    commit_ahead_r(C, c, x, r, p, alpha, rr_new);
    arrives(C, x->d, alpha, p->d);
    return;
  }
  if (c.outcome == XrOutcome::TrySpec) {
    if (C.fused.have_value && alpha_was_rr_over_pw(C, alpha, false)) {
      commit_spec_r(C, r, rr_new);  // (the speculated x / p half updates x in place: with the speculation there is no queue)
      if (C.lazy.depth != 1) broken("a queue beside the speculation");
      return;
    }
    drop_in_flight(C);
  }
  const int at = rr_next_at(C.iter);
  forget_fused(C);
  arrives(C, x->d, alpha, p->d);
  if (can_defer_x(C, x, r, p, w)) arm_deferred(C, x, p, alpha, false);
  else { flush_lazy(C); applies(C, x->d, alpha, p->d); }
  const bool p_ahead = ahead_wants_p(C, c, p);
  if (p_ahead) {
    C.ahead.slot = xpend_buffer(C);
    C.ahead_target = C.xpend.shadow[C.ahead.slot].buf;
    writes_p(C, C.ahead_target);
  }
  ++C.seq;
  calc_xr_ran(C, c, p_ahead, at, rr_new, x, r, p, w);
}

static void play_calc_p(Ctx &C, double beta) {
  abft_hip_vector *p = C.vec('p');
  const abft_hip_vector *r = C.vec('r');
  enter(C, KEEP_FLIGHT | KEEP_DEFERRED | KEEP_LAZY);
  const PCall c = classify_calc_p(C, p, r, beta);
  if (c.outcome == POutcome::CommitAhead) {
    if (C.xpend.shadow[C.ahead.slot].buf != C.ahead_target) broken("the run-ahead's buffer changed under it");
    commit_ahead_p(C, p);
    return;
  }
  if (c.outcome == POutcome::CommitSpec) { commit_spec_p(C, p); return; }
  const bool completes = completes_iteration(C, p, r);
  flush_xpend(C);
  forget_fused(C);
  bool taken = false;
  if (C.defer.active) {
    if (deferred_rides_with(C, p, r)) {
      C.defer.active = false;
      if (pending_can_take(C, p, r)) {
        const int at = xpend_buffer(C);
        writes_p(C, C.xpend.shadow[at].buf);
        adopt_p_leave_pending(C, p, at);
        taken = true;
      }
      C.xpend.last_p = p;
      if (!taken) { flush_lazy(C); applies(C, C.defer.x, C.defer.alpha, C.defer.p); }  // calc_px: x in place
    } else {
      flush_deferred(C);
    }
  }
  if (!taken) {
    flush_lazy(C);
    if (C.lazy.count) broken("a calc_p that took no update along left the queue filled");
  }
  calc_p_ran(C, c, completes, p, r);
}

static void shutdown(Ctx &C) {
  flush_lazy(C);
  flush_xpend(C);
  flush_deferred(C);
  if (!C.owed.empty()) broken("the context went with updates still owed");
  if (C.applied != C.arrived) broken("not every update was applied exactly once");
}

static void show(const Ctx &C) {
  printf("%ld %ld %ld %ld %ld %ld %ld %d %ld %ld %ld %d\n", C.ahead.commit_p, C.ahead.commit_r, C.ahead.drops,
         C.xpend.absorbed, C.xpend.flushed, C.spec.commits, C.spec.drops, (int)C.flight, C.lazy.bursts,
         C.lazy.applied_in_bursts, C.lazy.applied_by_flush, C.lazy.depth);
}

static void begin(Ctx &C, const char *xin, const char *ahead, const char *spec, const char *depth) {
  C = Ctx();
  for (int k = 0; k < 5; k++) {
    C.v[k].d = arena[k];
    C.v[k].n = N;
    C.v[k].root = &C.v[k];
  }
  static double scal[8];
  C.iter.scal = scal;
  C.xin_modes = ABFT_X_IN_SPMV_MODES;
  C.ahead.level = ABFT_AHEAD_DEFAULT;
  C.spec.enabled = spec[0] != '0';
  if (xin[0] != '-') {
    C.xin_enabled = xin[0] != '0';
    if (C.xin_enabled) C.xin_modes = ~0u;
  }
  if (ahead[0] != '-') C.ahead.level = ahead[0] == '2' ? 2 : ahead[0] == '1' ? 1 : 0;
  C.lazy.depth = depth[0] == '4' ? 4 : depth[0] == '2' ? 2 : 1;
  loop_settle_switches(C);
  C.configured = C.lazy.depth;
}

int main() {
  static Ctx C;
  char line[256], op[16], a[32], b[32], c[32], d[32];
  while (fgets(line, sizeof(line), stdin)) {
    a[0] = b[0] = c[0] = d[0] = 0;
    if (sscanf(line, "%15s %31s %31s %31s %31s", op, a, b, c, d) < 1) continue;
    const std::string o = op;
    if (o == "begin") begin(C, a, b, c, d);
    else if (o == "dot") play_dot(C, C.vec(a[0]), C.vec(b[0]), from_bits(c));
    else if (o == "spmv") play_spmv(C, 'p');
    else if (o == "spmv_q") play_spmv(C, 'q');
    else if (o == "xr") play_calc_xr(C, 'x', from_bits(a), from_bits(b));
    else if (o == "xr_q") play_calc_xr(C, 'q', from_bits(a), from_bits(b));
    else if (o == "p") play_calc_p(C, from_bits(a));
    else if (o == "other") enter(C, 0u);
    else if (o == "nomem") C.spares_left = atoi(a);
    else if (o == "show") show(C);
    else if (o == "end") { shutdown(C); show(C); }
    else { fprintf(stderr, "unknown step: %s", line); return 2; }
    ring_holds(C);
  }
  return 0;
}
