// device_buffers.h -- the one owner of an engine's device and pinned host memory (internal header).
// The engine keeps its typed raw pointers (the launch sites take them as they are); every allocation is registered here, release() frees one and clears the
// caller's pointer (a second upload frees and reallocates), and the destructor frees whatever is still registered.  Not thread-safe, like the engine itself.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

namespace nmfamd {

class DeviceBuffers {
public:
	DeviceBuffers() = default;
	DeviceBuffers(const DeviceBuffers&) = delete;
	DeviceBuffers& operator=(const DeviceBuffers&) = delete;
	~DeviceBuffers() { for (const Entry& e : owned_) free_entry(e); }

	// device memory; zero: filled with zero bytes on `stream`, in the order of the calls.  On failure *p stays nullptr.
	template <typename P>
	hipError_t device(P** p, size_t bytes, bool zero, hipStream_t stream) {
		void* q = nullptr;
		hipError_t e = hipMalloc(&q, bytes);
		if (e != hipSuccess) return e;
		owned_.push_back({q, false});
		*p = static_cast<P*>(q);
		return zero ? hipMemsetAsync(q, 0, bytes, stream) : hipSuccess;
	}
	// pinned host memory
	template <typename P>
	hipError_t pinned(P** p, size_t bytes) {
		void* q = nullptr;
		hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
		if (e != hipSuccess) return e;
		owned_.push_back({q, true});
		*p = static_cast<P*>(q);
		return hipSuccess;
	}
	// frees the buffers and clears the pointers; nullptr and pointers this owner does not hold are left alone
	template <typename... P>
	void release(P*&... p) { ((free_registered(p) ? void(p = nullptr) : void()), ...); }
	// a buffer of `from` becomes this owner's (scratch that turns out to be the result)
	void adopt(DeviceBuffers& from, const void* p) {
		for (size_t i = 0; i < from.owned_.size(); ++i)
			if (from.owned_[i].p == p) { owned_.push_back(from.owned_[i]); from.owned_.erase(from.owned_.begin() + (long)i); return; }
	}
	size_t count() const { return owned_.size(); }

private:
	struct Entry { void* p; bool host; };
	static void free_entry(const Entry& e) { if (e.host) (void)hipHostFree(e.p); else (void)hipFree(e.p); }
	bool free_registered(const void* p) {
		for (size_t i = 0; i < owned_.size(); ++i)
			if (owned_[i].p == p) { free_entry(owned_[i]); owned_.erase(owned_.begin() + (long)i); return true; }
		return false;
	}
	std::vector<Entry> owned_;
};

} // namespace nmfamd
