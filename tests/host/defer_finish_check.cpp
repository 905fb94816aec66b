// xr_can_defer_finish (loop_state.h) is asked BEFORE calc_xr's kernel goes out and must answer what ahead_wants_p
// answers AFTER it: otherwise calc_r would leave its finish to a calc_p that is never launched, or keep the ticket
// where the pair was known.  Every combination of what the two read, on four plain vectors: the same answer, and the
// same state left behind; never with the switch off; the switch settles to off where the run-ahead is off.
// Prints the number of combinations checked; exits 1 at the first difference.
#include <cstdio>

#include "loop_state.h"

int main() {
  static double buf[4][8];
  long checked = 0, yes = 0;
  for (unsigned m = 0; m < (1u << 10); m++) {
    abft_hip_vector x, r, p, w;
    abft_hip_vector *v[4] = {&x, &r, &p, &w};
    for (int k = 0; k < 4; k++) {
      v[k]->d = buf[k];
      v[k]->n = 8;
      v[k]->root = v[k];
    }
    LoopState L;
    L.ahead.level = 1;
    L.ahead.defer_finish = m & 1u;
    L.ahead.armed = m >> 1 & 1u;
    L.defer_enabled = m >> 2 & 1u;
    L.xin_enabled = m >> 3 & 1u;
    L.xpend.armed = m >> 4 & 1u;
    L.xpend.active = m >> 5 & 1u;
    L.capturing = m >> 6 & 1u;
    x.exposed = m >> 7 & 1u;
    if (m >> 8 & 1u) r.d = x.d + 4;  // r overlaps x: x += alpha p cannot be deferred
    XrCall c{XrOutcome::AsWritten, (m >> 9 & 1u) != 0, 1.0};
    const bool before = xr_can_defer_finish(L, c, &x, &r, &p, &w);
    LoopState after_as_written = L;
    // what xr_as_written does around the launch of calc_r / calc_xr
    if (can_defer_x(after_as_written, &x, &r, &p, &w)) arm_deferred(after_as_written, &x, &p, 0.5, false);
    const bool after = ahead_wants_p(after_as_written, c, &p);
    checked++;
    if (!L.ahead.defer_finish) {
      if (before) { printf("switch off, yet deferred: %u\n", m); return 1; }
      continue;
    }
    if (before != after) { printf("before %d, after %d: %u\n", before, after, m); return 1; }
    yes += before;
  }
  if (!yes) { printf("never deferred\n"); return 1; }
  for (int level = 0; level < 3; level++)
    for (int xin = 0; xin < 2; xin++) {
      LoopState L;
      L.ahead.level = level;
      L.ahead.defer_finish = true;
      L.xin_enabled = xin;
      loop_settle_switches(L);
      if (L.ahead.defer_finish != (L.ahead.level > 0)) { printf("settle: level %d xin %d\n", level, xin); return 1; }
    }
  printf("%ld %ld\n", checked, yes);
  return 0;
}
