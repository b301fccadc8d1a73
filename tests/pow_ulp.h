/* TEST INFRASTRUCTURE (tests/test_oracle_schemes.py): force-included into a second build of oracle/pop_oracle.c, it makes pow return
 * the neighbouring double, up or down, in POW_ULP_ONE_IN-th shares of its calls each (chosen by a hash of the argument), which is
 * what separates two correct math libraries.  The test measures how far one ulp of pow moves the oracle's own fields. */
#include <math.h>
#include <stdint.h>
#include <string.h>
static inline double pow_ulp(double a, double b) {
  const double r = pow(a, b);
  uint64_t u;
  memcpy(&u, &a, sizeof u);
  u ^= u >> 29; u *= 0x9E3779B97F4A7C15ull; u ^= u >> 32;
  const unsigned h = (unsigned)(u % POW_ULP_ONE_IN);
  if (h == 0) return nextafter(r, INFINITY);
  if (h == 1) return nextafter(r, -INFINITY);
  return r;
}
#define pow(a, b) pow_ulp(a, b)
