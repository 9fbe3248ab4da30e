// C ABI, direct exchange: K sharded over the GPUs of one node without a collective library call.  What travels between the
// ranks at set-up, the boxes this process owns, set-up and release; the exchange itself is k_finalize_exchange
// (mppi_update.h), launched by launch_update() in ccv_mppi_capi.hip.
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <mutex>

#include "capi_internal.h"

namespace {

// ---- what travels between the ranks at set-up, and the boxes this process owns --------------------------------------
struct ExchangeBlob {
    hipIpcMemHandle_t ipc;
    int32_t fine_grained;   // the box is fine-grained memory (coherent across devices)
    uint32_t nonce;         // rank 0's is the base of the sequence numbers
    int32_t pid;
    int32_t device;         // ordinal inside that process
    char bus[24];           // PCI bus id of the device that holds the box
};

// Boxes created by THIS process: hipIpcOpenMemHandle refuses a handle of the opening process itself, so a process that
// drives several handles (several devices from one process, or several shards on one device) maps them directly.
struct OwnBox {
    ExchangeBlob blob;
    ExchangeBox* box;
};
std::mutex g_box_mutex;
std::vector<OwnBox> g_boxes;

}  // namespace

namespace ccv {

void exchange_release(ccv_mppi_handle* h) {
    for (int r = 0; r < kMaxRanks; ++r) {
        if (h->box_opened[r] && h->box_peer[r]) (void)hipIpcCloseMemHandle(h->box_peer[r]);
        h->box_opened[r] = false;
        h->box_peer[r] = nullptr;
    }
    if (h->d_box) {
        {
            std::lock_guard<std::mutex> lock(g_box_mutex);
            g_boxes.erase(std::remove_if(g_boxes.begin(), g_boxes.end(), [&](const OwnBox& b) { return b.box == h->d_box; }), g_boxes.end());
        }
        (void)hipFree(h->d_box);
    }
    if (h->d_xvec) (void)hipFree(h->d_xvec);
    if (h->h_xflag) (void)hipHostFree(h->h_xflag);
    h->h_xflag = nullptr;
    if (h->pending_vec == h->d_xvec) h->pending_vec = nullptr;
    h->d_box = nullptr;
    h->d_xvec = nullptr;
    h->d_xflag = nullptr;
    h->xchg_connected = false;
    h->xchg_world = h->xchg_rank = 0;
}

// After a synchronisation: did the exchange kernel give up waiting for a peer?  The flag lives in pinned host-mapped memory
// (the kernel stores to it once, system scope, in the rare case): reading it costs no copy and no extra synchronisation.
// Sticky: the controls are NaN from then on; releasing the exchange (ccv_mppi_destroy, or a failed set-up) frees it and a
// new ccv_mppi_exchange_create starts from a cleared one.
int exchange_check(ccv_mppi_handle* h) {
    if (!h->h_xflag) return CCV_MPPI_OK;
    if (*static_cast<volatile int32_t*>(h->h_xflag)) {
        char msg[256];
        std::snprintf(msg, sizeof(msg), "direct exchange: a peer's partial vector did not arrive within %.3g s; the controls are NaN "
                                        "from that iteration on (destroy the handles and set the exchange up again)", h->xchg_timeout_s);
        return fail(h, CCV_MPPI_ERR_TIMEOUT, msg);
    }
    return CCV_MPPI_OK;
}

}  // namespace ccv

extern "C" {

int ccv_mppi_exchange_handle_bytes(void) { return (int)sizeof(ExchangeBlob); }

int ccv_mppi_exchange_create(ccv_mppi_handle* h, int32_t world, int32_t rank, void* ipc_handle_out) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!ipc_handle_out || world < 1 || world > kMaxRanks || rank < 0 || rank >= world)
        return fail(h, CCV_MPPI_ERR_INVALID_ARG, "exchange: 1 <= world <= 8, 0 <= rank < world");
    if (h->cfg.flags & CCV_MPPI_FLAG_MIN_SHIFT)
        return fail(h, CCV_MPPI_ERR_INVALID_ARG, "MIN_SHIFT needs a cross-device min; not supported with partials");
    if (h->d_box) return fail(h, CCV_MPPI_ERR_STATE, "exchange already created");
    const DeviceGuard guard(h->cfg.device);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // Fine-grained memory: a peer's stores become visible to a kernel that is already running on the owner.  Ordinary
    // (coarse-grained) device memory guarantees that only inside one device, so it is accepted as a fall-back only when
    // every rank's box lives on this same device (ccv_mppi_exchange_connect checks; a one-device rehearsal).
    void* box = nullptr;
    ExchangeBlob blob;
    std::memset(&blob, 0, sizeof(blob));
    hipError_t e = hipExtMallocWithFlags(&box, sizeof(ExchangeBox), hipDeviceMallocFinegrained);
    if (e == hipSuccess) e = hipIpcGetMemHandle(&blob.ipc, box);
    blob.fine_grained = e == hipSuccess ? 1 : 0;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (box) (void)hipFree(box);
        box = nullptr;
        HIP_TRY(h, hipMalloc(&box, sizeof(ExchangeBox)));
        e = hipIpcGetMemHandle(&blob.ipc, box);
        if (e != hipSuccess) {
            (void)hipFree(box);
            return fail(h, CCV_MPPI_ERR_HIP, "hipIpcGetMemHandle failed: no peer mapping on this system", e);
        }
    }
    h->d_box = static_cast<ExchangeBox*>(box);
    auto undo = [&](int code, const char* what, hipError_t err) {
        exchange_release(h);
        return fail(h, code, what, err);
    };
    if ((e = hipMemset(box, 0, sizeof(ExchangeBox))) != hipSuccess) return undo(CCV_MPPI_ERR_HIP, "hipMemset(box)", e);
    if ((e = hipMalloc(&h->d_xvec, (size_t)(h->R + 1) * sizeof(double))) != hipSuccess) return undo(CCV_MPPI_ERR_ALLOC, "hipMalloc(xvec)", e);
    if ((e = hipMemset(h->d_xvec, 0, (size_t)(h->R + 1) * sizeof(double))) != hipSuccess) return undo(CCV_MPPI_ERR_HIP, "hipMemset(xvec)", e);
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&h->h_xflag), sizeof(int32_t), hipHostMallocMapped)) != hipSuccess)
        return undo(CCV_MPPI_ERR_ALLOC, "hipHostMalloc(xflag)", e);
    *h->h_xflag = 0;
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_xflag), h->h_xflag, 0)) != hipSuccess)
        return undo(CCV_MPPI_ERR_HIP, "hipHostGetDevicePointer(xflag)", e);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return undo(CCV_MPPI_ERR_HIP, "hipDeviceSynchronize", e);
    blob.pid = (int32_t)getpid();
    blob.device = h->cfg.device;
    if (hipDeviceGetPCIBusId(blob.bus, (int)sizeof(blob.bus), h->cfg.device) != hipSuccess) std::snprintf(blob.bus, sizeof(blob.bus), "dev%d", h->cfg.device);
    blob.bus[sizeof(blob.bus) - 1] = 0;
    // sequence base: a job that is started again must not take the packets an earlier one left in a peer's box for its own
    const uint64_t now = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
    blob.nonce = (uint32_t)(now ^ (now >> 29) ^ ((uint64_t)blob.pid * 0x9E3779B97F4A7C15ull >> 17));
    h->xchg_nonce = blob.nonce;
    if (const char* tv = std::getenv("CCV_MPPI_EXCHANGE_TIMEOUT_MS")) {
        const long ms = std::atol(tv);
        if (ms > 0) h->xchg_timeout_ticks = (unsigned long long)ms * 100000ull;
    }
    h->xchg_timeout_s = (double)h->xchg_timeout_ticks * 1.0e-8;   // 100 MHz ticks
    h->box_fine_grained = blob.fine_grained != 0;
    h->xchg_world = world;
    h->xchg_rank = rank;
    h->xchg_seq = 0;
    {
        std::lock_guard<std::mutex> lock(g_box_mutex);
        g_boxes.push_back(OwnBox{blob, h->d_box});
    }
    std::memcpy(ipc_handle_out, &blob, sizeof(blob));
    return CCV_MPPI_OK;
}

int ccv_mppi_exchange_connect(ccv_mppi_handle* h, const void* ipc_handles) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!ipc_handles) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "ipc_handles is null");
    if (!h->d_box) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_exchange_create first");
    if (h->xchg_connected) return fail(h, CCV_MPPI_ERR_STATE, "exchange already connected");
    const DeviceGuard guard(h->cfg.device);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const ExchangeBlob* blobs = static_cast<const ExchangeBlob*>(ipc_handles);
    ExchangeBlob mine;
    std::memcpy(&mine, &blobs[h->xchg_rank], sizeof(mine));   // (the caller's buffer need not be aligned)
    auto undo = [&](int code, const char* what, hipError_t err) {
        for (int r = 0; r < kMaxRanks; ++r) {
            if (h->box_opened[r] && h->box_peer[r]) (void)hipIpcCloseMemHandle(h->box_peer[r]);
            h->box_opened[r] = false;
            h->box_peer[r] = nullptr;
        }
        return fail(h, code, what, err);
    };
    for (int r = 0; r < h->xchg_world; ++r) {
        ExchangeBlob peer;
        std::memcpy(&peer, reinterpret_cast<const char*>(ipc_handles) + (size_t)r * sizeof(ExchangeBlob), sizeof(peer));
        peer.bus[sizeof(peer.bus) - 1] = 0;
        if (r == h->xchg_rank) {
            h->box_peer[r] = h->d_box;
            continue;
        }
        if ((!peer.fine_grained || !mine.fine_grained) && std::strcmp(peer.bus, mine.bus) != 0)
            return undo(CCV_MPPI_ERR_STATE, "direct exchange refused: a box in coarse-grained memory would be polled across devices "
                                            "(fine-grained allocation or its IPC export failed); use the all-reduce path", hipSuccess);
        // a box of this very process (several handles driven by one process) is used as it is
        ExchangeBox* local = nullptr;
        if (peer.pid == (int32_t)getpid()) {
            std::lock_guard<std::mutex> lock(g_box_mutex);
            for (const OwnBox& b : g_boxes)
                if (std::memcmp(&b.blob.ipc, &peer.ipc, sizeof(peer.ipc)) == 0 && b.blob.nonce == peer.nonce) local = b.box;
        }
        if (local) {
            if (peer.device != h->cfg.device) {
                const hipError_t pe = hipDeviceEnablePeerAccess(peer.device, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) return undo(CCV_MPPI_ERR_HIP, "hipDeviceEnablePeerAccess", pe);
                (void)hipGetLastError();
            }
            h->box_peer[r] = local;
            continue;
        }
        void* p = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&p, peer.ipc, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return undo(CCV_MPPI_ERR_HIP, "hipIpcOpenMemHandle", e);
        h->box_peer[r] = static_cast<ExchangeBox*>(p);
        h->box_opened[r] = true;
        // touch the mapping through the runtime first: a mapping that cannot be used fails here with an error code
        // instead of faulting in a kernel
        unsigned long long probe = 0;
        if ((e = hipMemcpy(&probe, p, sizeof(probe), hipMemcpyDeviceToHost)) != hipSuccess) return undo(CCV_MPPI_ERR_HIP, "peer box not readable", e);
    }
    ExchangeBlob first;
    std::memcpy(&first, ipc_handles, sizeof(first));
    h->xchg_base = first.nonce;
    h->xchg_connected = true;
    return CCV_MPPI_OK;
}

int ccv_mppi_exchange_info(const ccv_mppi_handle* h, int32_t* world, int32_t* rank, int32_t* fine_grained, int32_t* connected) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (world) *world = h->xchg_world;
    if (rank) *rank = h->xchg_rank;
    if (fine_grained) *fine_grained = (h->d_box && h->box_fine_grained) ? 1 : 0;
    if (connected) *connected = h->xchg_connected ? 1 : 0;
    return CCV_MPPI_OK;
}

int ccv_mppi_iterate_exchange_enqueue(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref,
                                      const double* y_ref, double yaw_ref0, uint64_t seed, uint64_t iter) {
    int rc = check_iter_args(h, x0, dt, x_ref, y_ref);
    if (rc) return rc;
    if (!h->xchg_connected) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_exchange_create / _connect first");
    return enqueue_iteration(h, x0, dt, x_ref, y_ref, yaw_ref0, seed, iter, false, nullptr, false, true);
}

}  // extern "C"
