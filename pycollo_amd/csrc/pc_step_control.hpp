// The step controller of one node interval [ca, cb] of the propagation kernels (pc_solution.hpp: prop_walk).
// Pure arithmetic on scalars: no model, no arrays, no HIP.  It compiles with a plain C++ compiler too, and
// tests/c/step_control_sanitize.cpp runs it under AddressSanitizer + UBSan against scripted outcomes.
//
//   StepControl<K> s;
//   s.start_adaptive(ca, cb)  or  s.start_fixed(ca, cb, m);
//   while (s.more(max_steps)) {
//     ... one attempt of width s.h from s.c; it ends at s.end() ...
//     accepted = s.report(newton_ok, bad, err, on_accept);   // on_accept(): called, before c and h move on, if it is
//   }
//   s.failed(): the interval has not arrived; s.n_acc, s.n_rej, s.n_newton are its step counts.
//
// K holds the method's constants: K::exponent(), the power of err in the factor, and K::newton, whether an attempt can
// fail in its Newton iteration (report's newton_ok is not read without it).
//   adaptive: h starts as the whole interval.  An attempt is accepted when it is not bad and err <= 1;
//     factor = 0.2 when bad, 5 at err = 0, else min(5, max(0.2, 0.9 err^exponent)), at most 1 right after a rejection,
//     0.25 after a Newton failure (which rejects and counts in n_rej and n_newton); next h = min(h factor, the rest of
//     the interval), and the step that takes the rest ends at cb itself.  The interval fails when max_steps attempts
//     (accepted + rejected) have not brought it to cb.
//   fixed: m steps; step q starts at ca + q h0, h0 = (cb - ca) / m (computed, not accumulated); the last one has width
//     cb - its start and ends at cb.  max_steps is not read.  A Newton failure ends the interval as failed: the failed
//     attempt is its one rejected (and Newton-rejected) step.
#ifndef PC_STEP_CONTROL_HPP
#define PC_STEP_CONTROL_HPP

#include <math.h>

#ifndef PC_HD
#ifdef __HIPCC__
#define PC_HD __host__ __device__
#else
#define PC_HD
#endif
#endif
#define PC_STEP_FN PC_HD inline __attribute__((always_inline))

namespace pc {

struct StepDopri5 {   // the explicit 5(4) pair
  static PC_STEP_FN constexpr double exponent() { return -0.2; }
  static constexpr bool newton = false;
};
// The implicit method of order 4 with an estimate of order 3.  No kernel is built on it yet: pc_sol_propagate_stiff
// (pc_solution.hpp) still carries this control in its own body, and only the host test runs StepControl<StepSdirk4>
// and its Newton branches.  What ties the two together until the kernel moves is that both follow DESIGN 8h.
struct StepSdirk4 {
  static PC_STEP_FN constexpr double exponent() { return -0.25; }
  static constexpr bool newton = true;
};

template <class K>
struct StepControl {
  double c, h;                     // the next attempt: its start and its width
  bool last, after_reject, done;   // the attempt reaches cb; the one before it was rejected; the interval has arrived
  int n_acc, n_rej, n_newton;      // accepted, rejected (Newton failures included), rejected by a Newton failure
  double ca, cb, h0;               // the interval; fixed mode: the width of every step but the last
  int m;                           // fixed mode: the number of steps
  bool fixed;

  PC_STEP_FN void start_adaptive(double ca_, double cb_) {
    start(ca_, cb_, 0, false);
    h0 = cb - ca;
    c = ca;
    h = h0;
    last = true;
  }
  PC_STEP_FN void start_fixed(double ca_, double cb_, int m_) {
    start(ca_, cb_, m_, true);
    h0 = (cb - ca) / (double)m;
    place();
  }
  // the interval without a step: the counts of an interval behind a failure
  PC_STEP_FN void clear() { n_acc = n_rej = n_newton = 0; }

  PC_STEP_FN bool more(int max_steps) const { return !done && (fixed ? n_rej == 0 : n_acc + n_rej < max_steps); }
  PC_STEP_FN double end() const { return last ? cb : c + h; }
  PC_STEP_FN bool failed() const { return !done; }

  // the attempt from c of width h gave (newton_ok, bad, err); true: it is accepted.  Either way c, h are the next
  // attempt's afterwards.  (on_accept runs inside, where the kernels advanced their state before there was a
  // controller: with the caller acting on the returned flag instead, the implicit kernel took up to 25 more VGPRs.)
  template <class F>
  PC_STEP_FN bool report(bool newton_ok, bool bad, double err, F&& on_accept) {
    const bool ok = !K::newton || newton_ok;
    if (fixed) {
      if (!ok) {
        ++n_rej;
        ++n_newton;
        return false;
      }
      ++n_acc;
      on_accept();
      done = n_acc == m;
      if (!done) place();
      return true;
    }
    double factor = ok ? 0.2 : 0.25;
    if (ok && !bad) factor = err == 0.0 ? 5.0 : fmin(5.0, fmax(0.2, 0.9 * pow(err, K::exponent())));
    if (ok && !bad && err <= 1.0) {
      ++n_acc;
      on_accept();
      c = end();
      if (after_reject) factor = fmin(factor, 1.0);
      after_reject = false;
      const double rest = cb - c;
      if (last || !(rest > 0.0)) {
        done = true;
      } else {
        h *= factor;
        last = h >= rest;
        if (last) h = rest;
      }
      return true;
    }
    ++n_rej;
    if (!ok) ++n_newton;
    h *= factor;
    last = false;
    after_reject = true;
    return false;
  }

 private:
  PC_STEP_FN void start(double ca_, double cb_, int m_, bool fixed_) {
    ca = ca_;
    cb = cb_;
    m = m_;
    fixed = fixed_;
    after_reject = done = false;
    clear();
  }
  PC_STEP_FN void place() {   // fixed mode: step n_acc
    c = ca + (double)n_acc * h0;
    last = n_acc == m - 1;
    h = last ? cb - c : h0;
  }
};

}  // namespace pc

#endif  // PC_STEP_CONTROL_HPP
