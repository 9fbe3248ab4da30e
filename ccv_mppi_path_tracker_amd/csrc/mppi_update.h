// The small kernels around the rollout: weighted update (k_update_partials / k_finalize / k_finalize_exchange /
// k_apply_partials), re-derivation of the controls from the stored normals, MIN_SHIFT re-weighting and the read-back
// helpers.  No entry point is a template: every kernel is DEFINED in one translation unit, k_update.hip; this header has the argument
// structs and the declarations through which the host units of the C ABI (capi_internal.h) launch them.  The rollout
// kernels' translation units (k_*.hip) include mppi_launch.h and their family's header (mppi_rollout_*.h), not this one.
#pragma once
#include "mppi_kernels.h"
#include "mppi_top_weights.h"

namespace ccv {

// u = clamp(double(z) * sigma + u*[n]) for every sample and row, from the normals the fused iteration stored: for the
// stage-wise calls after a fused iteration and for the unfused update (MIN_SHIFT).  Same operations as the samplers.
struct MaterializeArgs {
    const float* z;
    const double* nominal_used;
    double* u;
    double sigma;
    double umin[5], umax[5];
    int32_t K, pitch, R, udim, zero_dim;   // zero_dim: the control dimension that steer_off forces to 0 (fb:517), or -1
};
__global__ void k_materialize_controls(MaterializeArgs A);   // grid (ceil(K / kBlock), R)

// ---- weighted update -------------------------------------------------------------------------------------------
struct UpdateArgs {
    const double* u;
    const double* w;
    const double* cost;
    double* partial;   // [(R+1)][nchunks]
    double* statpart;  // [nchunks][3]: min cost, max cost, zero-weight count
    int32_t K, pitch, R, nchunks;
};
// grid (nchunks, R+1).  Row n < R: sum_k w_k*u[n][k] over this chunk; row R: sum_k w_k (+ cost stats).
__global__ void k_update_partials(UpdateArgs A);
__global__ void k_update_partials_batch(UpdateArgs A, int kpad);   // batch handles (the plain kernel's iteration): grid (nchunks, R+1, B)

struct FinalizeArgs {
    const double* partial;   // [(R+1)][nchunks]
    const double* statpart;  // [nchunks][3]
    double* nominal;         // [R]      (mode 0)
    double* vec;             // [1+R]    unnormalised [sum w, sum w*u] (always written)
    double* stats;           // [4]      sum_w, min cost, max cost, zero-weight count
    int32_t R, nchunks, normalise;
    // Blocking calls (ccv_mppi_iterate, ccv_mppi_update): the result also goes straight into a mailbox in pinned host
    // memory, slot n = u*[n] for n < R, slots R .. R+3 = the four statistics.  A value travels as two self-validating 8-byte
    // packets {32 data bits, 32-bit sequence number}, each one atomic store (the exchange's packet format, below): the host
    // polls until every packet carries this call's number -- no copy engine, no stream synchronisation, no fence.  Null: off.
    unsigned long long* mail;
    uint32_t mail_seq;       // never 0
};
constexpr int finalize_blocks(int R) { return (R + 2 + kBlock / 64 - 1) / (kBlock / 64); }   // waves: R rows, sum w, statistics
__global__ void k_finalize(FinalizeArgs A);                  // grid finalize_blocks(R)
__global__ void k_finalize_batch(FinalizeArgs A, int fused);   // grid (finalize_blocks(R), B)
// batch handles in shifted-weight mode (ccv_mppi_batch_set_min_shift): k_finalize_batch over the SHIFT rollout kernels'
// block-relative partials, rescaled column by column with exp(-(m_g - m) / lambda_b); P: the parameter table [B], K: samples
// per instance (the zero-weight count of a workgroup whose scale is 0)
__global__ void k_finalize_batch_shift(FinalizeArgs A, const BatchParams* P, int K);   // grid (finalize_blocks(R), B)

// ---- K sharded over the GPUs of one node without a collective library call ---------------------------
// The exchanged message is 1 + (H-1)*u_dim doubles (<= 3.2 KB): far below the size at which a ring all-reduce pays, and a
// collective kernel launch between two rollout launches costs more than the transfer.  Instead every device owns an
// ExchangeBox in its HBM that all peers have mapped (hipIpc, xGMI peer access).  The wave of k_finalize_exchange that owns
// a row writes its value straight into slot [rank][row] of every peer's box, waits for the peers' values of the same row
// in its own box and adds them in rank order -- the same order on every device, so all devices hold the same bits.
// A value travels as two self-validating 8-byte packets {32 data bits, 32-bit sequence number} (each an atomic store):
// the receiver needs no flag and the sender no fence -- a packet is either the old one or the new one.  Two parities
// alternate: a slot is rewritten two exchanges later, which a peer can only reach after it has received this device's
// next packets, i.e. after this device's launch that read the slot has finished (stream order).
constexpr int kMaxRanks = 8;
constexpr int kMaxVec = 1 + (kMaxH - 1) * CCV_MPPI_MAX_UDIM;
struct ExchangeBox {
    unsigned long long pkt[2][kMaxRanks][kMaxVec][2];   // [parity][source rank][slot: 0 = sum w, 1 + row][high / low half]
};
struct ExchangeArgs {
    ExchangeBox* peer[kMaxRanks];   // every rank's box as mapped on this device (peer[rank] = the local one)
    ExchangeBox* local;
    double* reduced;                // [1 + R]: sum over ranks, rank order (becomes the deferred warm-start update)
    uint32_t seq;                   // this exchange's sequence number, never 0
    int32_t world, rank, parity;
    unsigned long long timeout_ticks;   // s_memrealtime ticks (100 MHz) to wait for the peers; then `reduced` is NaN
    int32_t* timeout_flag;              // set to 1 when that happens (the host reports it at the next synchronisation)
};
__global__ void k_finalize_exchange(FinalizeArgs A, ExchangeArgs X);   // grid finalize_blocks(R)
// After the cross-device all-reduce of [sum w, sum w*u]: u* = V / S on every device.
__global__ void k_apply_partials(const double* vec, double* nominal, double* stats, int R);

// ---- optional underflow-safe weights (CCV_MPPI_FLAG_MIN_SHIFT; not reference behaviour) --------------------------
__global__ void k_min_cost(const double* cost, int K, double* out_min);   // one workgroup of 1024
__global__ void k_reweight(const double* cost, const double* cmin, double lambda, int K, double* w);
// batch handles in shifted-weight mode, plain family: instance minima [B] and the weights around them (per-instance lambda)
__global__ void k_min_cost_batch(const double* cost, int K, int kpad, double* out_min);   // grid B, workgroups of 1024
__global__ void k_reweight_batch(const double* cost, const double* cmin, const BatchParams* P, int K, int kpad, double* w);   // grid (ceil(K / kBlock), B)

// ---- read-back helpers -----------------------------------------------------------------------------------------
// out[c][t][2] = (xs[t][first + c*stride], ys[t][...])
__global__ void k_gather_xy(const double* xs, const double* ys, int pitch, int H, int first, int count, int stride, double* out);
// top-N candidates by weight: one workgroup of kTopBlock running top_weights(); top_order_pairs() sorts the N pairs on the
// host (both, the key and kTopBlock: mppi_top_weights.h)
__global__ void k_top_weights(const double* w, int K, int N, int* idx_out, double* w_out);
// gather of listed samples: out[c][t] = (x, y) of sample idx[c] at step t
__global__ void k_gather_xy_list(const double* xs, const double* ys, int pitch, int H, const int* idx, int count, double* out);
__global__ void k_normalise_weights(const double* w, const double* stats, int first, int count, double* out);
// ... of one instance of a batch in shifted-weight mode (fused kernels): w[k] * s_g / S from the block-relative weights
__global__ void k_normalise_weights_shift(const double* w, const double* statpart, const double* stats, double lambda, int first,
                                          int count, double* out);

}  // namespace ccv
