// What the host side of the C ABI owns on the device, by type (capi_internal.h: the handles' parts hold these; capi_exchange.hip
// alone keeps its memory by hand, its box is opened and closed through IPC handles).  Move-only holders with no policy: a
// destructor that gives the resource back, moves that leave the source empty.  A setter builds its new arrays as locals, returns
// on a failure (the locals free themselves) and move-assigns them into the handle on success, where the old ones go.
// Call sites read the pointer through the implicit conversion (d_x + n, a kernel argument, a hipMemcpy operand); get() is for
// the places the language does not convert: reinterpret_cast and ->.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

namespace ccv {

// one hipMalloc allocation of n T
template <typename T>
class DeviceArray {
  public:
    DeviceArray() = default;
    DeviceArray(const DeviceArray&) = delete;
    DeviceArray& operator=(const DeviceArray&) = delete;
    DeviceArray(DeviceArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DeviceArray& operator=(DeviceArray&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    ~DeviceArray() { reset(); }
    // an empty holder only (hipErrorInvalidValue otherwise: an allocation is never dropped by allocating over it)
    hipError_t alloc(const size_t n) { return p_ ? hipErrorInvalidValue : hipMalloc(&p_, n * sizeof(T)); }
    // ... and a hipMemset, which may still run when this returns: the caller synchronises before a kernel of another stream reads
    hipError_t alloc_zeroed(const size_t n) {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(p_, 0, n * sizeof(T));
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    T* p_ = nullptr;
};

// one hipHostMalloc allocation of n T, with the flags the caller gives
template <typename T>
class PinnedArray {
  public:
    PinnedArray() = default;
    PinnedArray(const PinnedArray&) = delete;
    PinnedArray& operator=(const PinnedArray&) = delete;
    PinnedArray(PinnedArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    PinnedArray& operator=(PinnedArray&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    ~PinnedArray() { reset(); }
    hipError_t alloc(const size_t n, const unsigned flags) { return p_ ? hipErrorInvalidValue : hipHostMalloc(&p_, n * sizeof(T), flags); }
    // the address the device reads and writes the same memory at
    hipError_t device(T** out) const { return hipHostGetDevicePointer(reinterpret_cast<void**>(out), p_, 0); }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    T* p_ = nullptr;
};

// one event: an ordering mark (hipEventDisableTiming), or with `timing` one hipEventElapsedTime can read
class Event {
  public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t create(const bool timing = false) {
        if (e_) return hipErrorInvalidValue;
        return timing ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, hipEventDisableTiming);
    }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }

  private:
    hipEvent_t e_ = nullptr;
};

// a handle's own stream (DeviceBuffers::own_stream): declared before every array and event of the handle, so it goes last
class Stream {
  public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s_) (void)hipStreamDestroy(s_);
    }
    hipError_t create() { return s_ ? hipErrorInvalidValue : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    operator hipStream_t() const { return s_; }

  private:
    hipStream_t s_ = nullptr;
};

static_assert(!std::is_copy_constructible<DeviceArray<double>>::value && !std::is_copy_constructible<PinnedArray<double>>::value &&
                  !std::is_copy_constructible<Event>::value && !std::is_copy_constructible<Stream>::value,
              "an owner is not copied");
static_assert(std::is_nothrow_move_constructible<DeviceArray<double>>::value && std::is_nothrow_move_assignable<DeviceArray<double>>::value &&
                  std::is_nothrow_move_constructible<PinnedArray<double>>::value && std::is_nothrow_move_assignable<PinnedArray<double>>::value &&
                  std::is_nothrow_move_constructible<Event>::value && std::is_nothrow_move_assignable<Event>::value,
              "a setter commits by move, and a vector of events grows by it");
static_assert(sizeof(DeviceArray<double>) == sizeof(double*), "a holder is its pointer");

// Pinned staging in rotation: n slots of `bytes` each in one allocation, an event per slot.  A slot is refilled only after the
// work that last read it has run: take() waits for the slot's event if the slot was used -- the call's only wait -- and seal()
// records it after the last reader.  Slot::device: the same bytes as kernels address them, for a mapped ring (null otherwise:
// the reader is a hipMemcpyAsync from Slot::host).
struct Slot {
    int index;
    uint8_t* host;
    const uint8_t* device;
};

class StagingRing {
  public:
    // idempotent: a ring that exists stays as it is
    hipError_t create(const int n, const size_t bytes, const bool mapped) {
        if (mem_) return hipSuccess;
        PinnedArray<uint8_t> mem;
        uint8_t* dev = nullptr;
        std::vector<Event> ev((size_t)n);
        if (hipError_t e = mem.alloc((size_t)n * bytes, hipHostMallocDefault)) return e;
        if (mapped) {
            if (hipError_t e = mem.device(&dev)) return e;
        }
        for (Event& v : ev)
            if (hipError_t e = v.create()) return e;
        mem_ = std::move(mem);
        dev_ = dev;
        ev_ = std::move(ev);
        used_.assign((size_t)n, 0);
        bytes_ = bytes;
        next_ = 0;
        return hipSuccess;
    }
    // the next slot, free to be filled
    hipError_t take(Slot& s) {
        const int i = next_;
        next_ = (i + 1) % (int)ev_.size();
        if (used_[(size_t)i]) {
            if (hipError_t e = hipEventSynchronize(ev_[(size_t)i])) return e;
        }
        s = Slot{i, mem_ + (size_t)i * bytes_, dev_ ? dev_ + (size_t)i * bytes_ : nullptr};
        return hipSuccess;
    }
    // after the last enqueue that reads the slot (launched: its result, hipGetLastError() after a kernel launch)
    hipError_t seal(const Slot& s, const hipError_t launched, const hipStream_t stream) {
        used_[(size_t)s.index] = 1;
        return launched != hipSuccess ? launched : hipEventRecord(ev_[(size_t)s.index], stream);
    }
    explicit operator bool() const { return (bool)mem_; }

  private:
    PinnedArray<uint8_t> mem_;
    const uint8_t* dev_ = nullptr;   // (a view: mem_ as the device addresses it)
    std::vector<Event> ev_;
    std::vector<uint8_t> used_;
    size_t bytes_ = 0;
    int next_ = 0;
};

}  // namespace ccv
