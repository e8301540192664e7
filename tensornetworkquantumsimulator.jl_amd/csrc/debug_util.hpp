// debug_util.hpp -- what the kernel-level test entry points (debug_*.cpp, include/tnqs_debug.h) share: host arrays in, host arrays out.
// Every entry point is defined once, where its body is, as extern "C" int tnqs_dbg_x(...) { return guard([&] { ... }); } -- the header is included here, so the
// compiler checks each definition against its declaration.
#pragma once
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "api_guard.hpp"
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "launch_util.hpp"
#include "../../include/tnqs_debug.h"

namespace tnqs {
struct DBuf { void* p = nullptr; explicit DBuf(size_t n) { HIPCHK(hipMalloc(&p, n ? n : 1)); } ~DBuf() { (void)hipFree(p); }
              void up(const void* h, size_t n) { if (n) HIPCHK(hipMemcpy(p, h, n, hipMemcpyHostToDevice)); } void down(void* h, size_t n) { if (n) HIPCHK(hipMemcpy(h, p, n, hipMemcpyDeviceToHost)); } };
// a descriptor array on the device: DevItems<T> d(n) allocates room for n items and d.up(items) sends them, DevItems<T> d(items) does both; d.get() is what the launch takes
template <class T> struct DevItems : DBuf {
    explicit DevItems(size_t n) : DBuf(sizeof(T) * n) {}
    explicit DevItems(const std::vector<T>& v) : DBuf(sizeof(T) * v.size()) { up(v); }
    void up(const std::vector<T>& v) { DBuf::up(v.data(), sizeof(T) * v.size()); }
    void up(const T& one) { DBuf::up(&one, sizeof(T)); }
    const T* get() const { return (const T*)p; }
};
inline void up_ints(DBuf& d, const int* h, size_t n) { d.up(h, sizeof(int) * n); }
inline void need_gpu() { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Err(TNQS_ERR_HIP, "no HIP device available"); }

inline bool is_dtype(int dtype) { return dtype == TNQS_C64 || dtype == TNQS_C128; }
inline size_t esz_of(int dtype) { return dtype == TNQS_C64 ? 8 : 16; }
// the launch written once for both element types: by_dtype(dtype, [&](auto t) { launch_x<decltype(t)>(...); }) with t a float (TNQS_C64) or a double
template <class F> void by_dtype(int dtype, F&& f) { if (dtype == TNQS_C64) f(float{}); else f(double{}); }

// the items' arrays one after the other: off[i] = where item i starts, off[n] = the total
template <class F> void cat_offsets(int n, std::vector<size_t>& off, F&& size_of) { off.assign(n + 1, 0); for (int i = 0; i < n; ++i) off[i + 1] = off[i] + size_of(i); }

// a device array of slots that start at 256-byte multiples (the engine's sub-buffers); the gaps keep a 0xff filling that is checked after the launch, so a
// kernel that writes past its slot is reported instead of going unnoticed.  Plain slots (no guard) are filled with put() and sent with up().
// With guard_bytes the array is an output as the caller hands it over: guard band, item 0, guard band, item 1, ..., guard band.  On the device every item has the band
// that follows it right behind it (the leading band right in front of item 0).  The whole array goes up as the caller filled it (up(src)) and comes back whole
// (down(dst, what)), so a write outside an item shows in a guard band or is reported here
struct Slots {
    size_t gb, total; std::vector<size_t> off, len; std::vector<char> host; std::unique_ptr<DBuf> dev;
    explicit Slots(size_t guard_bytes = 0) : gb(guard_bytes), total(round256(guard_bytes)) {}
    void add(size_t bytes) { off.push_back(total); len.push_back(bytes); total += round256(bytes + gb); }
    void alloc() { host.assign(total ? total : 1, (char)0xff); dev.reset(new DBuf(total)); }
    void put(size_t i, const void* src) { std::memcpy(host.data() + off[i], src, len[i]); }
    void get(size_t i, void* dst) const { std::memcpy(dst, host.data() + off[i], len[i]); }
    char* at(size_t i) const { return (char*)dev->p + off[i]; }
    void up() { dev->up(host.data(), total); }
    void up(const void* src) { caller(const_cast<void*>(src), false); up(); }
    void down(const char* what) { fetch(std::string("dbg: a kernel wrote past the end of a slot of ") + what); }
    void down(void* dst, const char* what) { fetch(std::string("dbg: a kernel wrote outside an item of ") + what); caller(dst, true); }
private:
    void fetch(const std::string& complaint) {
        dev->down(host.data(), total);
        auto gap = [&](size_t b0, size_t b1) { for (size_t b = b0; b < b1; ++b) if (host[b] != (char)0xff) throw Err(TNQS_ERR_INVALID, complaint); };
        gap(0, round256(gb) - gb);
        for (size_t i = 0; i < off.size(); ++i) gap(off[i] + len[i] + gb, off[i] + round256(len[i] + gb));
    }
    void caller(void* arr, bool out) {      // between the caller's contiguous array (bands included) and the slots
        char* p = (char*)arr;
        auto move = [&](char* h, size_t n) { if (out) std::memcpy(p, h, n); else std::memcpy(h, p, n); p += n; };
        move(host.data() + round256(gb) - gb, gb);
        for (size_t i = 0; i < off.size(); ++i) move(host.data() + off[i], len[i] + gb);
    }
};
using Guarded = Slots;      // an output array with guard bands: Guarded g(guard_bytes)
// several Slots at once, in the order given (the order of the device allocations)
template <class... S> void alloc_all(S&... s) { (s.alloc(), ...); }
template <class... S> void up_all(S&... s) { (s.up(), ...); }
// input arrays: the items one after the other on the host, 256-byte aligned slots on the device
inline void put_all(Slots& s, const void* src) { const char* p = (const char*)src; for (size_t i = 0; i < s.off.size(); ++i) { s.put(i, p); p += s.len[i]; } }
// the argument check of the entry points over nitems items of bond dimension n[i] with a guard of guard_elems elements
inline void post_check(const char* who, int dtype, int nitems, const int* n, int guard_elems) {
    if (!is_dtype(dtype) || nitems < 1 || !n || guard_elems < 0) throw Err(TNQS_ERR_INVALID, std::string(who) + ": bad arguments");
    for (int i = 0; i < nitems; ++i) {
        if (n[i] < 1) throw Err(TNQS_ERR_INVALID, std::string(who) + ": n >= 1");
        if (n[i] > 256) throw Err(TNQS_ERR_UNSUPPORTED, std::string(who) + ": bond dimension > 256");
    }
}
}  // namespace tnqs
