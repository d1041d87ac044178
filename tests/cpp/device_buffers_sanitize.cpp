// Stand-alone driver of csrc/device_buffers.h for the sanitizer run of tests/test_engine_plan.py: the five HIP entry points the owner calls are defined HERE on
// malloc / free (no GPU, no HIP runtime linked), with a ledger of what is live, so that AddressSanitizer sees every leak, double free and write past a buffer.
#include "../../nmfgpu_amd/csrc/device_buffers.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

static std::set<void*> g_device, g_host;
static long g_fills = 0;
static bool g_fail_next = false;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
	if (g_fail_next) { g_fail_next = false; return hipErrorOutOfMemory; }
	*p = std::malloc(bytes ? bytes : 1);
	g_device.insert(*p);
	return hipSuccess;
}
hipError_t hipFree(void* p) {
	if (g_device.erase(p) != 1) { std::printf("hipFree of a pointer that is not a live device buffer\n"); std::abort(); }
	std::free(p);
	return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
	*p = std::malloc(bytes ? bytes : 1);
	g_host.insert(*p);
	return hipSuccess;
}
hipError_t hipHostFree(void* p) {
	if (g_host.erase(p) != 1) { std::printf("hipHostFree of a pointer that is not a live pinned buffer\n"); std::abort(); }
	std::free(p);
	return hipSuccess;
}
hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t) {
	std::memset(p, value, bytes);
	++g_fills;
	return hipSuccess;
}
}

#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main() {
	using nmfamd::DeviceBuffers;
	float *a = nullptr, *b = nullptr, *pin = nullptr;
	int* idx = nullptr;
	{
		DeviceBuffers own;
		// allocate: plain, zero-filled, pinned
		CHECK(own.device(&a, 1000 * sizeof(float), false, nullptr) == hipSuccess && a != nullptr);
		CHECK(own.device(&b, 77 * sizeof(float), true, nullptr) == hipSuccess && g_fills == 1);
		for (int i = 0; i < 77; ++i) CHECK(b[i] == 0.f);
		a[999] = 1.f;
		CHECK(own.pinned(&pin, 64) == hipSuccess && pin != nullptr);
		CHECK(own.device(&idx, 10 * sizeof(int), false, nullptr) == hipSuccess);
		CHECK(own.count() == 4 && g_device.size() == 3 && g_host.size() == 1);
		// a failed allocation registers nothing and leaves the pointer alone
		float* none = nullptr;
		g_fail_next = true;
		CHECK(own.device(&none, 16, true, nullptr) == hipErrorOutOfMemory && none == nullptr && own.count() == 4 && g_fills == 1);
		// release: several typed pointers at once, cleared; a second release and a foreign pointer are no-ops
		own.release(a, idx);
		CHECK(a == nullptr && idx == nullptr && own.count() == 2 && g_device.size() == 1);
		own.release(a, idx);
		float on_stack = 0.f, *foreign = &on_stack;
		own.release(foreign);
		CHECK(foreign == &on_stack && own.count() == 2);
		// re-allocate into the released pointers (a second upload), release the pinned buffer
		CHECK(own.device(&a, 10 * sizeof(float), true, nullptr) == hipSuccess && a != nullptr && a[9] == 0.f);
		CHECK(own.device(&idx, 3 * sizeof(int), false, nullptr) == hipSuccess);
		own.release(pin);
		CHECK(pin == nullptr && g_host.empty());
		CHECK(own.pinned(&pin, 8) == hipSuccess);
		// scratch that turns out to be the result: moved to the other owner, which then frees it exactly once
		{
			DeviceBuffers scratch;
			int *keep = nullptr, *drop = nullptr;
			CHECK(scratch.device(&keep, 40, false, nullptr) == hipSuccess && scratch.device(&drop, 40, false, nullptr) == hipSuccess);
			own.adopt(scratch, keep);
			CHECK(scratch.count() == 1 && own.count() == 5);
			keep[9] = 7;
		}
		CHECK(g_device.size() == 4);      // b, a, idx, keep: `drop` went with its owner
		// destruction with live buffers: device and pinned
		CHECK(own.count() == 5);
	}
	CHECK(g_device.empty() && g_host.empty());
	std::printf("ok\n");
	return 0;
}
