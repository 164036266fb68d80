// libumx device memory: the arena every device buffer of a trainer, training set, labeler and inference context comes from, and its
// debug guard mode (umx_internal.h: DevArena).
#include "umx_internal.h"

#include <cstdlib>

namespace umx {

// ---- the device memory of a trainer / training set (umx_internal.h) ----
int arena_init(DevArena* a, std::string* why) {
    a->fill = -1;
    const char* e = getenv("UMX_DEBUG_GUARD");
    if (!e || !*e) return UMX_OK;
    char* end = nullptr;
    const long v = strtol(e, &end, 0);
    if (*end || v < 0 || v > 255) {
        *why = std::string("UMX_DEBUG_GUARD=") + e + ": the fill must be one byte (0..255, e.g. 0xff)";
        return UMX_ERR_INVALID;
    }
    a->fill = (int)v;
    return UMX_OK;
}

hipError_t arena_alloc(DevArena* a, void** out, size_t bytes, bool zero, const char* label, bool scoped) {
    bytes = std::max<size_t>(16, bytes);
    void* d = nullptr;
    if (a->fill < 0) {
        hipError_t e = hipMalloc(&d, bytes);
        if (e != hipSuccess) return e;
        a->allocs.push_back(d);
        if (zero && (e = hipMemset(d, 0, bytes)) != hipSuccess) return e;
        *out = d;
        return hipSuccess;
    }
    // a zone at least as large as the buffer: an index off by a whole image / plane / row lands in it, not in unmapped memory
    const size_t zone = std::max<size_t>(64 << 10, (bytes + 4095) / 4096 * 4096);
    hipError_t e = hipMalloc(&d, zone + bytes + zone);
    if (e != hipSuccess) return e;
    a->allocs.push_back(d);
    char* p = static_cast<char*>(d);
    if ((e = hipMemset(p, a->fill, zone + bytes + zone)) != hipSuccess) return e;
    if (zero && (e = hipMemset(p + zone, 0, bytes)) != hipSuccess) return e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return e;   // (the trainer's streams do not wait for the null stream)
    while (*label == '&') ++label;
    a->blocks.push_back({d, zone, bytes, zone, std::string(label) + " (#" + std::to_string(a->serial++) + ")", scoped});
    *out = p + zone;
    return hipSuccess;
}

hipError_t arena_release(DevArena* a, void* p) {
    void* base = p;
    for (size_t i = 0; i < a->blocks.size(); ++i)
        if (static_cast<char*>(a->blocks[i].base) + a->blocks[i].front == p) {
            base = a->blocks[i].base;
            a->blocks.erase(a->blocks.begin() + i);
            break;
        }
    const auto it = std::find(a->allocs.begin(), a->allocs.end(), base);
    if (it == a->allocs.end()) return hipErrorInvalidValue;   // not this arena's
    a->allocs.erase(it);
    return hipFree(base);
}

hipError_t arena_refill(const DevArena& a, hipStream_t stream) {
    if (a.fill < 0) return hipSuccess;
    for (const DevBlock& b : a.blocks) {
        if (!b.scoped) continue;
        const hipError_t e = hipMemsetAsync(static_cast<char*>(b.base) + b.front, a.fill, b.bytes, stream);
        if (e != hipSuccess) return e;
    }
    return hipStreamSynchronize(stream);
}

int arena_check(const DevArena& a, std::string* msg) {
    if (a.fill < 0) return UMX_OK;
    std::vector<uint8_t> h;
    char buf[512];
    for (const DevBlock& b : a.blocks) {
        for (int side = 0; side < 2; ++side) {
            const size_t n = side ? b.back : b.front;
            const char* src = static_cast<const char*>(b.base) + (side ? b.front + b.bytes : 0);
            h.resize(n);
            const hipError_t e = hipMemcpy(h.data(), src, n, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                *msg = std::string("guard check: hipMemcpy failed: ") + hipGetErrorString(e);
                return UMX_ERR_HIP;
            }
            const int rc = umx_guard_scan(h.data(), n, side, b.bytes, a.fill, b.label.c_str(), buf, sizeof buf);
            if (rc != UMX_OK) {
                *msg = buf;
                return rc;
            }
        }
    }
    return UMX_OK;
}

void arena_free(DevArena* a) {
    for (void* p : a->allocs) (void)hipFree(p);
    a->allocs.clear();
    a->blocks.clear();
}

}  // namespace umx

extern "C" {

int umx_guard_scan(const uint8_t* zone, size_t zone_bytes, int side, size_t buf_bytes, int fill, const char* label, char* msg,
                   size_t cap) {
    if (!zone || !label || (side != 0 && side != 1)) return UMX_ERR_INVALID;
    size_t first = SIZE_MAX, last = 0;
    for (size_t j = 0; j < zone_bytes; ++j)
        if (zone[j] != (uint8_t)fill) {
            if (first == SIZE_MAX) first = j;
            last = j;
        }
    if (first == SIZE_MAX) return UMX_OK;
    // offsets from the first byte of the buffer: the front zone ends at -1, the back zone starts at buf_bytes
    const long long o1 = side ? (long long)(buf_bytes + first) : (long long)first - (long long)zone_bytes;
    const long long o2 = side ? (long long)(buf_bytes + last) : (long long)last - (long long)zone_bytes;
    if (msg && cap)
        snprintf(msg, cap, "guard: %s (%zu bytes): the %s red zone was written, bytes %lld .. %lld of the buffer (fill 0x%02x)", label,
                 buf_bytes, side ? "back" : "front", o1, o2, fill & 0xff);
    return UMX_ERR_GUARD;
}

}  // extern "C"
