// The sizing core of the scratch carver (scratch.h): plain C++17, no HIP header, so a host-only
// program can include it and check it under sanitizers.
//
// A scratch buffer's layout is stated once, as a layout function: a callable taking `Carver &` that
// assigns one pointer per region through take<T>(count) and stages host arrays through up(). carve_with
// runs it twice -- on a measuring carver, to learn the size, then on a live carver over the buffer
// that size was ensured for -- so the size can never undercount what is carved.
//
// A layout function runs twice: it only assigns pointers and calls take / up. No std::swap, no memset,
// no launch, no size query that touches the device, nothing that reads through a carved pointer (the
// measuring pass hands out nullptr).
#pragma once
#include <cstddef>
#include <cstdint>

namespace corro {

inline size_t al256(size_t bytes) { return (bytes + 255) / 256 * 256; }

struct Carver {
    // the host-to-device copy of a staged array; false on failure. Null: the caller's arrays are
    // device memory and up() hands them through.
    typedef bool (*Copy)(void *arg, void *dst, const void *src, size_t bytes);

    uint8_t *base = nullptr;   // live mode only; a measuring carver has none
    bool live = false;
    size_t used = 0;           // the offset of the next region: the buffer's size after the last take
    Copy copy = nullptr;
    void *copy_arg = nullptr;
    bool ok = true;            // sticky: false once a copy has failed

    // The next region: count elements of T, rounded up to 256 bytes. nullptr when measuring (the base
    // is added to the offset only in live mode, never to a null pointer).
    template <class T> T *take(size_t count) {
        const size_t at = used;
        used += al256(count * sizeof(T));
        return live ? reinterpret_cast<T *>(base + at) : nullptr;
    }

    // A caller's input array of `bytes` bytes: device memory is handed through unchanged; host memory
    // gets a region of `room` >= bytes bytes and, in live mode, its asynchronous copy.
    template <class T> T *up(T *src, size_t bytes, size_t room) {
        if (!copy) return src;
        uint8_t *dst = take<uint8_t>(room);
        if (live && bytes && !copy(copy_arg, dst, src, bytes)) ok = false;
        return reinterpret_cast<T *>(dst);
    }
};

// ensure(bytes, &base): make the buffer hold `bytes` bytes and give its address; nonzero on failure
// (returned as is). *copies_ok (optional) is cleared when a staged copy failed.
template <class Ensure, class Layout>
int carve_with(Ensure &&ensure, Layout &&layout, Carver::Copy copy = nullptr, void *copy_arg = nullptr, bool *copies_ok = nullptr) {
    Carver m;
    m.copy = copy;
    layout(m);
    Carver c;
    if (int rc = ensure(m.used, &c.base)) return rc;
    c.live = true;
    c.copy = copy;
    c.copy_arg = copy_arg;
    layout(c);
    if (!c.ok && copies_ok) *copies_ok = false;
    return 0;
}

}  // namespace corro
