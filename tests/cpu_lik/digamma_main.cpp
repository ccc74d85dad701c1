// digamma() of csrc/lik_math.hpp on the host, on its own: reads arguments (hex or decimal floats) from the command line, or one
// per line from standard input when there are none, and prints psi(x) as a hex float, one per line.
// tests/test_lik_math_cpu.py compares the output with mpmath.
#include <cstdio>
#include <cstdlib>

#include "lik_math.hpp"

int main(int argc, char** argv) {
  if (argc > 1) {
    for (int i = 1; i < argc; ++i) std::printf("%a\n", digamma(std::strtod(argv[i], nullptr)));
    return 0;
  }
  char line[128];
  while (std::fgets(line, sizeof line, stdin)) {
    char* end = nullptr;
    const double x = std::strtod(line, &end);
    if (end == line) continue;
    std::printf("%a\n", digamma(x));
  }
  return 0;
}
