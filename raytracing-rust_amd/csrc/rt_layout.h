// rt_layout.h -- how one device buffer is carved into parts: the ONE place in librt_hip.so that adds sizes up into offsets.
// A bump allocator over offsets, not over memory: the caller describes the parts in order and keeps a handle per part; once the
// buffer holds total() bytes and `base` is set (grow_device_buffer, rt_api_internal.h) the same handles resolve to typed
// pointers, so the size of a buffer and every pointer into it come from the same sequence of calls.  Every part starts 16-byte
// aligned (the workspaces of the denoiser, display, bloom and depth-of-field stages need it).  An optional part (its host pointer
// NULL) takes no room and resolves to nullptr.  Offsets are 64-bit: a frame of 2^31 pixels lays out without wrapping.  Fixed
// capacity, no heap: a description beyond it sets `overflowed` and resolves to nullptr (grow_device_buffer refuses it).
// HIP-free: tests/cpp/layout_check.cpp includes it alone.
#pragma once
#include <cstdint>

namespace rt {

struct Layout {
	static constexpr int kCapacity = 16;
	template <class T> struct Part { int index; }; // -1: described beyond the capacity

	uint64_t offset[kCapacity], size[kCapacity]; // bytes; an absent part has size 0
	int n = 0;
	uint64_t end = 0; // a multiple of 16
	bool overflowed = false;
	char *base = nullptr; // the buffer, once it holds total() bytes

	// `count` elements of T, if `present`
	template <class T> Part<T> add(uint64_t count, bool present = true)
	{
		if (n == kCapacity) {
			overflowed = true;
			return Part<T>{-1};
		}
		offset[n] = end;
		size[n] = present ? count * sizeof(T) : 0;
		end += (size[n] + 15u) / 16u * 16u;
		return Part<T>{n++};
	}
	// `count` elements of T if the caller gave `host`
	template <class T> Part<T> optional(const void *host, uint64_t count) { return add<T>(count, host != nullptr); }
	Part<char> bytes(uint64_t count) { return add<char>(count); }

	uint64_t total() const { return end; }
	template <class T> uint64_t size_of(Part<T> p) const { return p.index < 0 ? 0 : size[p.index]; }
	template <class T> T *at(Part<T> p) const { return size_of(p) ? reinterpret_cast<T *>(base + offset[p.index]) : nullptr; }
};

} // namespace rt
