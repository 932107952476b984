// One-kernel probe: the error of the device tanh, as the step kernel's policy
// calls it, against a long-double tanh on the host.  Built by tools/tanh_probe.py
// with the compiler flags of the model code objects (fp32, or fp64 with
// -DDMC_REAL_IS_DOUBLE), so that the library function is lowered the same way.
//
//   tanh_probe FILE      FILE: raw array of `real` (the pre-activations)
// prints: <count> <max |dev - ref| / u> <x at the maximum>, u = eps(real)/2.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#ifdef DMC_REAL_IS_DOUBLE
typedef double real;
#else
typedef float real;
#endif

__global__ void tanh_kernel(const real* x, real* y, int n) {
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i < n) y[i] = tanh(x[i]);
}

#define TRY(expr)                                                                  \
  do {                                                                             \
    hipError_t err_ = (expr);                                                      \
    if (err_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(err_));                 \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: tanh_probe FILE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<real> x;
  real buf[4096];
  for (size_t got; (got = fread(buf, sizeof(real), 4096, f)) > 0;) x.insert(x.end(), buf, buf + got);
  fclose(f);
  const int n = (int)x.size();
  if (n == 0) { fprintf(stderr, "no values\n"); return 2; }
  real *dx = nullptr, *dy = nullptr;
  TRY(hipMalloc((void**)&dx, n*sizeof(real)));
  TRY(hipMalloc((void**)&dy, n*sizeof(real)));
  TRY(hipMemcpy(dx, x.data(), n*sizeof(real), hipMemcpyHostToDevice));
  tanh_kernel<<<(n + 255)/256, 256>>>(dx, dy, n);
  TRY(hipGetLastError());
  std::vector<real> y(n);
  TRY(hipMemcpy(y.data(), dy, n*sizeof(real), hipMemcpyDeviceToHost));
  const long double u = std::numeric_limits<real>::epsilon()/2.0L;
  long double worst = 0, at = 0;
  for (int i = 0; i < n; i++) {
    const long double e = fabsl((long double)y[i] - tanhl((long double)x[i]))/u;
    if (e > worst) { worst = e; at = x[i]; }
  }
  printf("%d %.4Lf %.9Lg\n", n, worst, at);
  (void)hipFree(dx);
  (void)hipFree(dy);
  return 0;
}
