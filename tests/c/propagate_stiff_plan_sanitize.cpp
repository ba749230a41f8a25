// CPU-only sanitizer harness for the host side of the implicit propagation (TEST INFRASTRUCTURE).
//
// Compiles pc_propagate_plan.hpp under g++ -fsanitize=address,undefined and
//   1. feeds check_propagate_stiff_options every option set it is given and prints "ok" or the refusal;
//   2. for NY = 1 .. PC_SOL_STIFF_MAX_NY walks what the lanes of one workgroup of pc_sol_propagate_stiff touch in their
//      two LDS arrays (the factors, element e of lane l at [e * 64 + l], and the row swaps) with bounds-checked accesses,
//      as the kernel's LU does: every element written, every pivot row in [k, NY), rows swapped whole.  Every address is
//      owned by exactly one (lane, element) pair, none lies beyond the array, and the two arrays fit the static LDS of
//      a workgroup (64 KiB).
//
//   usage: propagate_stiff_plan_sanitize <in.txt> <out.txt>
//   in.txt: n_cases, then per case: substeps rtol max_steps newton_max NY atol[max(NY, 0)] with_atol
//           (rtol / atol may be nan or inf; with_atol = 0 passes a null pointer)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../pycollo_amd/csrc/pc_propagate_plan.hpp"

namespace {

double real(std::istream& in) {   // (operator>> does not read "nan" / "inf")
  std::string tok;
  in >> tok;
  return std::strtod(tok.c_str(), nullptr);
}

// the LDS columns of one workgroup for NY states; returns the number of addresses touched
long long walk_lds(int NY, std::ostream& out) {
  const int TB = PC_SOL_PROP_TB;
  const size_t n_lu = (size_t)NY * NY * TB, n_piv = (size_t)NY * TB;
  std::vector<double> lu(n_lu, -1.0);
  std::vector<int32_t> piv(n_piv, -1);
  std::vector<int32_t> owner_lu(n_lu, -1), owner_piv(n_piv, -1);
  if (pcs::stiff_lds_bytes(NY) != (int64_t)(n_lu * sizeof(double) + n_piv * sizeof(int32_t))) throw std::runtime_error("lds bytes");
  if (pcs::stiff_lds_bytes(NY) > 65536) throw std::runtime_error("the arrays pass 64 KiB");
  long long touched = 0;
  for (int lane = 0; lane < TB; ++lane) {
    // the kernel's fill: a matrix that makes every pivot search pick a lane-dependent row
    for (int r = 0; r < NY; ++r)
      for (int c = 0; c < NY; ++c) {
        const int64_t at = pcs::stiff_lu_index(r * NY + c, lane);
        if (owner_lu.at((size_t)at) != -1) throw std::runtime_error("two elements share an address");
        owner_lu.at((size_t)at) = lane * NY * NY + r * NY + c;
        lu.at((size_t)at) = (r == c ? 1.0 : 0.0) + 0.01 * (double)(((r + lane) % NY) * NY + c + 1) * ((r + c + lane) % 3 == 0 ? -1.0 : 1.0);
        ++touched;
      }
    // the factorisation's accesses, bounds-checked
    auto L = [&](int r, int c) -> double& { return lu.at((size_t)pcs::stiff_lu_index(r * NY + c, lane)); };
    for (int k = 0; k < NY; ++k) {
      int p = k;
      double best = std::fabs(L(k, k));
      for (int r = k + 1; r < NY; ++r)
        if (std::fabs(L(r, k)) > best) {
          best = std::fabs(L(r, k));
          p = r;
        }
      if (p < k || p >= NY) throw std::runtime_error("pivot row out of range");
      const int64_t at = pcs::stiff_piv_index(k, lane);
      if (owner_piv.at((size_t)at) != -1) throw std::runtime_error("two row swaps share an address");
      owner_piv.at((size_t)at) = lane * NY + k;
      piv.at((size_t)at) = p;
      ++touched;
      if (p != k)
        for (int c = 0; c < NY; ++c) std::swap(L(k, c), L(p, c));
      const double d = L(k, k);
      if (d == 0.0) throw std::runtime_error("zero pivot in the walk's matrix");
      for (int r = k + 1; r < NY; ++r) {
        const double l = L(r, k) / d;
        L(r, k) = l;
        for (int c = k + 1; c < NY; ++c) L(r, c) = L(r, c) - l * L(k, c);
      }
    }
    // the solve's reads: every swap, every factor
    double sum = 0.0;
    for (int k = 0; k < NY; ++k) {
      const int p = piv.at((size_t)pcs::stiff_piv_index(k, lane));
      if (p < k || p >= NY) throw std::runtime_error("stored pivot row out of range");
      for (int c = 0; c < NY; ++c) sum += L(k, c);
    }
    if (!(sum == sum)) throw std::runtime_error("the walk's factors are not finite");
  }
  for (size_t i = 0; i < n_lu; ++i)
    if (owner_lu[i] == -1) throw std::runtime_error("an element of the factor array is owned by no lane");
  for (size_t i = 0; i < n_piv; ++i)
    if (owner_piv[i] == -1) throw std::runtime_error("an entry of the swap array is owned by no lane");
  // lanes that read the same element read consecutive words
  for (int e = 0; e < NY * NY; ++e)
    for (int lane = 1; lane < TB; ++lane)
      if (pcs::stiff_lu_index(e, lane) != pcs::stiff_lu_index(e, lane - 1) + 1) throw std::runtime_error("lanes are not consecutive");
  out << "lds " << NY << ' ' << n_lu << ' ' << n_piv << ' ' << pcs::stiff_lds_bytes(NY) << ' ' << touched << '\n';
  return touched;
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
  for (int ic = 0; ic < n_cases; ++ic) {
    long long substeps, max_steps, newton_max;
    int NY, with_atol;
    in >> substeps;
    const double rtol = real(in);
    in >> max_steps >> newton_max >> NY;
    std::vector<double> atol((size_t)(NY > 0 ? NY : 0));
    for (auto& a : atol) a = real(in);
    in >> with_atol;
    try {
      pcs::check_propagate_stiff_options(substeps, rtol, with_atol ? atol.data() : nullptr, NY, max_steps, newton_max);
      out << "case " << ic << " ok\n";
    } catch (const std::exception& e) {
      out << "case " << ic << " refused " << e.what() << '\n';
    }
  }
  out << "max_ny " << PC_SOL_STIFF_MAX_NY << " max_newton " << PC_SOL_STIFF_MAX_NEWTON << " tb " << PC_SOL_PROP_TB << '\n';
  try {
    for (int NY = 1; NY <= PC_SOL_STIFF_MAX_NY; ++NY) walk_lds(NY, out);
  } catch (const std::exception& e) {
    out << "lds failed " << e.what() << '\n';
    return 1;
  }
  if (pcs::stiff_lds_bytes(PC_SOL_STIFF_MAX_NY + 1) <= 65536) {
    out << "lds failed the limit is not the largest NY that fits\n";
    return 1;
  }
  return 0;
}
