// Timer (not part of the library): the stand-alone r = 64 launch of the Gauss-Jordan inverse (csrc/inverse_gj64.h, one workgroup of eight waves), float and
// double, one HIP event pair per launch, median over the launches after a warm-up.  The body is whichever inverse_gj64.h the include path finds first, so that
// tools/time_inverse.sh can build the header of another revision beside the tree's and run the two in turn (docs/INVERSE.md has the figures).
//   time_inverse [launches = 200] [warm-up = 50]
// Prints one line per type: median, minimum and 90th percentile in microseconds, and max |X A - I| of the last result.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "inverse_gj64.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <typename T>
__global__ __launch_bounds__(512) void k_inverse(const T* __restrict__ A, int RP, int r, T* __restrict__ Ainv, T offdiag, T diag) {
	nmfamd::inverse_gj64_body<T>(A, RP, r, Ainv, offdiag, diag);
}

template <typename T>
static int run(const char* name, int launches, int warmup) {
	const int r = 64;
	// W^T W of 256 x 64 uniform values (a fixed linear congruential sequence): the normal matrix of the least-squares algorithms
	std::vector<double> W(256 * r), G(r * r, 0.0);
	unsigned long long s = 12345;
	for (double& w : W) { s = s * 6364136223846793005ull + 1442695040888963407ull; w = (double)(s >> 40) / (double)(1ull << 24); }
	for (int i = 0; i < r; ++i) for (int j = 0; j < r; ++j) { double a = 0; for (int k = 0; k < 256; ++k) a += W[k * r + i] * W[k * r + j]; G[j * r + i] = a; }
	std::vector<T> hA(r * r), hX(r * r);
	for (int e = 0; e < r * r; ++e) hA[e] = (T)G[e];
	T *dA = nullptr, *dX = nullptr;
	CHECK(hipMalloc(&dA, sizeof(T) * r * r));
	CHECK(hipMalloc(&dX, sizeof(T) * r * r));
	CHECK(hipMemcpy(dA, hA.data(), sizeof(T) * r * r, hipMemcpyHostToDevice));
	std::vector<hipEvent_t> e0(launches), e1(launches);
	for (int i = 0; i < launches; ++i) { CHECK(hipEventCreate(&e0[i])); CHECK(hipEventCreate(&e1[i])); }
	for (int i = 0; i < warmup; ++i) hipLaunchKernelGGL((k_inverse<T>), dim3(1), dim3(512), 0, nullptr, dA, r, r, dX, (T)-0.01, (T)0.5);
	CHECK(hipDeviceSynchronize());
	for (int i = 0; i < launches; ++i) {
		CHECK(hipEventRecord(e0[i], nullptr));
		hipLaunchKernelGGL((k_inverse<T>), dim3(1), dim3(512), 0, nullptr, dA, r, r, dX, (T)-0.01, (T)0.5);
		CHECK(hipEventRecord(e1[i], nullptr));
	}
	CHECK(hipDeviceSynchronize());
	std::vector<float> us(launches);
	for (int i = 0; i < launches; ++i) { float ms = 0; CHECK(hipEventElapsedTime(&ms, e0[i], e1[i])); us[i] = ms * 1e3f; CHECK(hipEventDestroy(e0[i])); CHECK(hipEventDestroy(e1[i])); }
	std::sort(us.begin(), us.end());
	CHECK(hipMemcpy(hX.data(), dX, sizeof(T) * r * r, hipMemcpyDeviceToHost));
	double worst = 0;
	for (int i = 0; i < r; ++i) for (int j = 0; j < r; ++j) {
		double a = 0;
		for (int k = 0; k < r; ++k) a += (double)hX[k * r + i] * ((double)(T)(hA[j * r + k] + (k == j ? (T)0.5 : (T)-0.01)));
		worst = std::max(worst, std::fabs(a - (i == j ? 1.0 : 0.0)));
	}
	std::printf("%-6s r = 64  median %.2f us  min %.2f  p90 %.2f  (%d launches)  max |X A - I| %.2e\n", name, us[launches / 2], us[0], us[(launches * 9) / 10], launches, worst);
	CHECK(hipFree(dA));
	CHECK(hipFree(dX));
	return 0;
}

int main(int argc, char** argv) {
	const int launches = argc > 1 ? std::max(1, std::atoi(argv[1])) : 200, warmup = argc > 2 ? std::max(0, std::atoi(argv[2])) : 50;
	if (run<float>("float", launches, warmup)) return 1;
	return run<double>("double", launches, warmup);
}
