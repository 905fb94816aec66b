// loop_state_play.cpp -- the host-scalar CG loop's decisions (abft_sparse_cg_amd/csrc/loop_state.h) played without a
// GPU: this program stands where abft_hip.hip stands.  Every launch and allocation succeeds, every scalar a reduction
// would publish comes from the script, the vectors are handles onto an arena nobody reads.  tests/test_loop_state_host.py
// builds it with -fsanitize=address,undefined and feeds it scripts on stdin, any number of them:
//
//   begin XIN AHEAD SPEC   the switches as abft_hip_init reads them: ABFT_HIP_X_IN_SPMV (0, 1, - unset), ABFT_HIP_AHEAD
//                          (0, 1, 2, - unset), ABFT_HIP_SPECULATE (0, 1); the matrix is of ECC mode `none`
//   dot A B BITS           abft_hip_dot(A, B); BITS: what the reduction publishes, were it run (a double's 16 hex digits)
//   spmv                   abft_hip_spmv(A, p, w) on the streaming CSR layout, whole, with the fused product
//   xr ALPHA RR_NEW        abft_hip_calc_xr(x, r, p, w, ALPHA); RR_NEW: the r.r its reduction -- run now, ahead, or
//                          speculated -- publishes
//   p BETA                 abft_hip_calc_p(p, r, BETA)
//   other                  an entry point with no flags (abft_hip_vector_map of x, say)
//   show                   print committed_p committed_r dropped absorbed flushed spec_commits spec_drops in_flight
//   end                    show, and the context is gone
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "loop_state.h"

#ifndef ABFT_AHEAD_DEFAULT
#error "build with -DABFT_AHEAD_DEFAULT=... -DABFT_X_IN_SPMV_MODES=... as abft_internal.h has them"
#endif

static const int N = 8;
static double arena[16][N + 2];  // x, r, p, w, q, then the shadows as they are asked for

struct Ctx : LoopState {
  abft_hip_vector v[5];
  int next_buf = 5;
  uint32_t seq = 0;
  abft_hip_vector *vec(char c) { return &v[c == 'x' ? 0 : c == 'r' ? 1 : c == 'p' ? 2 : c == 'w' ? 3 : 4]; }
};

static double from_bits(const char *s) {
  const unsigned long long u = strtoull(s, nullptr, 16);
  double d;
  memcpy(&d, &u, sizeof(d));
  return d;
}

static void shadow_ensure(Ctx &C, Shadow &s) {
  if (s.buf && s.n == N) return;
  if (C.next_buf >= 16) abort();
  s.buf = arena[C.next_buf++];
  s.n = N;
}
static int xpend_buffer(Ctx &C) {
  const int at = pending_shadow_slot(C.xpend, N);
  shadow_ensure(C, C.xpend.shadow[at]);
  C.xpend.shadow_at = at;
  return at;
}

static void enter(Ctx &C, unsigned keep) {
  prologue_begin(C, keep);
  if (prologue_flushes_pending(keep)) (void)pending_flush_due(C);
  if (prologue_flushes_deferred(keep)) (void)deferred_flush_due(C);
  prologue_end(C, keep);
}

static void play_dot(Ctx &C, const abft_hip_vector *a, const abft_hip_vector *b, double published) {
  enter(C, KEEP_FLIGHT);
  if (fused_serves_dot(C, a, b, false)) {
    if (!C.fused.have_value) fused_value_read(C, published);
    return;
  }
  drop_in_flight(C);
  fused_slot_reused(C);
  rr_handed(C.iter, rr_next_at(C.iter), published);
  ++C.seq;
}

static void play_spmv(Ctx &C) {
  const abft_hip_vector *vec = C.vec('p'), *result = C.vec('w');
  enter(C, KEEP_PENDING);
  const bool eligible = pending_path_on(C, 0u);
  const bool absorb = pending_absorbed_by(C, eligible, vec, result);
  if (!absorb) (void)pending_flush_due(C);
  forget_fused(C);
  if (absorb) pending_absorbed(C);
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
  }
}

static void play_calc_xr(Ctx &C, double alpha, double rr_new) {
  abft_hip_vector *x = C.vec('x'), *r = C.vec('r'), *p = C.vec('p'), *w = C.vec('w');
  enter(C, KEEP_FLIGHT);
  const XrCall c = classify_calc_xr(C, x, r, p, w, alpha);
  if (c.outcome == XrOutcome::CommitAhead) {
    commit_ahead_r(C, c, x, r, p, alpha, rr_new);
    return;
  }
  if (c.outcome == XrOutcome::TrySpec) {  // (the fused p.w was read by the dot(p, w) before: every script asks for it)
    if (C.fused.have_value && alpha_was_rr_over_pw(C, alpha, false)) {
      commit_spec_r(C, r, rr_new);
      return;
    }
    drop_in_flight(C);
  }
  const int at = rr_next_at(C.iter);
  forget_fused(C);
  if (can_defer_x(C, x, r, p, w)) arm_deferred(C, x, p, alpha, false);
  const bool p_ahead = ahead_wants_p(C, c, p);
  if (p_ahead) C.ahead.slot = xpend_buffer(C);
  ++C.seq;
  calc_xr_ran(C, c, p_ahead, at, rr_new, x, r, p, w);
}

static void play_calc_p(Ctx &C, double beta) {
  abft_hip_vector *p = C.vec('p');
  const abft_hip_vector *r = C.vec('r');
  enter(C, KEEP_FLIGHT | KEEP_DEFERRED);
  const PCall c = classify_calc_p(C, p, r, beta);
  if (c.outcome == POutcome::CommitAhead) { commit_ahead_p(C, p); return; }
  if (c.outcome == POutcome::CommitSpec) { commit_spec_p(C, p); return; }
  const bool completes = completes_iteration(C, p, r);
  (void)pending_flush_due(C);
  forget_fused(C);
  if (C.defer.active) {
    if (deferred_rides_with(C, p, r)) {
      C.defer.active = false;
      if (pending_can_take(C, p, r)) adopt_p_leave_pending(C, p, xpend_buffer(C));
      C.xpend.last_p = p;
    } else {
      (void)deferred_flush_due(C);
    }
  }
  calc_p_ran(C, c, completes, p, r);
}

static void show(const Ctx &C) {
  printf("%ld %ld %ld %ld %ld %ld %ld %d\n", C.ahead.commit_p, C.ahead.commit_r, C.ahead.drops, C.xpend.absorbed,
         C.xpend.flushed, C.spec.commits, C.spec.drops, (int)C.flight);
}

static void begin(Ctx &C, const char *xin, const char *ahead, const char *spec) {
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
  loop_settle_switches(C);
}

int main() {
  static Ctx C;
  char line[256], op[16], a[32], b[32], c[32];
  while (fgets(line, sizeof(line), stdin)) {
    a[0] = b[0] = c[0] = 0;
    if (sscanf(line, "%15s %31s %31s %31s", op, a, b, c) < 1) continue;
    const std::string o = op;
    if (o == "begin") begin(C, a, b, c);
    else if (o == "dot") play_dot(C, C.vec(a[0]), C.vec(b[0]), from_bits(c));
    else if (o == "spmv") play_spmv(C);
    else if (o == "xr") play_calc_xr(C, from_bits(a), from_bits(b));
    else if (o == "p") play_calc_p(C, from_bits(a));
    else if (o == "other") enter(C, 0u);
    else if (o == "show" || o == "end") show(C);
    else { fprintf(stderr, "unknown step: %s", line); return 2; }
  }
  return 0;
}
