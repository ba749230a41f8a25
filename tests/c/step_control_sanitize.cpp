// CPU-only sanitizer harness for the step controller of the propagation kernels (TEST INFRASTRUCTURE).
//
// Compiles pc_step_control.hpp under g++ -fsanitize=address,undefined and drives StepControl through scripted outcomes
// of the attempts of one node interval, as prop_walk (pc_solution.hpp) drives it: start, then while more(): the attempt's
// c, h and end(), then report(newton_ok, bad, err).  An attempt behind the script's last outcome gets the last outcome
// again.  Every double is printed as a hex float.
//
//   usage: step_control_sanitize <in.txt> <out.txt>
//   in.txt: n_cases, then per case: exponent (5: -1/5, 4: -1/4)  newton (0 / 1)  m (0: adaptive)  ca cb  max_steps
//           n_outcomes, then n_outcomes times: newton_ok bad err   (doubles as hex floats, "nan" or "inf")
//   out.txt, per case: "case <i>", per attempt "attempt <c> <h> <ce> <last> <accepted> <on_accept calls so far>", then
//           "end <c> <n_acc> <n_rej> <n_newton> <failed>"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../pycollo_amd/csrc/pc_step_control.hpp"

namespace {

// the two combinations the kernels do not use: every script runs with both exponents
struct StepDopri5Newton : pc::StepDopri5 {
  static constexpr bool newton = true;
};
struct StepSdirk4Plain : pc::StepSdirk4 {
  static constexpr bool newton = false;
};

double real(std::istream& in) {   // (operator>> reads neither hex floats nor "nan" / "inf")
  std::string tok;
  in >> tok;
  return std::strtod(tok.c_str(), nullptr);
}

struct Outcome {
  int newton_ok, bad;
  double err;
};

std::string hex(double x) {
  char buf[64];
  std::snprintf(buf, sizeof(buf), "%a", x);
  return buf;
}

template <class K>
void run(int m, double ca, double cb, int max_steps, const std::vector<Outcome>& script, std::ostream& out) {
  pc::StepControl<K> s;
  if (m > 0) s.start_fixed(ca, cb, m);
  else s.start_adaptive(ca, cb);
  size_t at = 0;
  int calls = 0;
  const long long bound = (long long)(m > 0 ? m : max_steps) + 1;   // the controller's own bound, and one attempt more
  for (long long attempts = 0; s.more(max_steps); ++attempts) {
    if (attempts >= bound) throw std::runtime_error("the controller asks for more attempts than its bound");
    const Outcome& o = script.at(at);
    if (at + 1 < script.size()) ++at;
    out << "attempt " << hex(s.c) << ' ' << hex(s.h) << ' ' << hex(s.end()) << ' ' << (int)s.last;
    const bool accepted = s.report(o.newton_ok != 0, o.bad != 0, o.err, [&] { ++calls; });
    out << ' ' << (int)accepted << ' ' << calls << '\n';
  }
  out << "end " << hex(s.c) << ' ' << s.n_acc << ' ' << s.n_rej << ' ' << s.n_newton << ' ' << (int)s.failed() << '\n';
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <in.txt> <out.txt>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::ofstream out(argv[2]);
  int n_cases = 0;
  in >> n_cases;
  try {
    for (int ic = 0; ic < n_cases; ++ic) {
      int exponent, newton, m, max_steps, n_out;
      in >> exponent >> newton >> m;
      const double ca = real(in), cb = real(in);
      in >> max_steps >> n_out;
      if (!in || n_out < 1) throw std::runtime_error("malformed case");
      std::vector<Outcome> script((size_t)n_out);
      for (auto& o : script) {
        in >> o.newton_ok >> o.bad;
        o.err = real(in);
      }
      out << "case " << ic << '\n';
      if (exponent == 5 && !newton) run<pc::StepDopri5>(m, ca, cb, max_steps, script, out);
      else if (exponent == 5) run<StepDopri5Newton>(m, ca, cb, max_steps, script, out);
      else if (exponent == 4 && newton) run<pc::StepSdirk4>(m, ca, cb, max_steps, script, out);
      else if (exponent == 4) run<StepSdirk4Plain>(m, ca, cb, max_steps, script, out);
      else throw std::runtime_error("unknown exponent");
    }
  } catch (const std::exception& e) {
    out << "failed " << e.what() << '\n';
    return 1;
  }
  return 0;
}
