// runtime.h -- host-side device runtime shared by the C ABI (abi.cpp) and the
// prover orchestrator (prover.cpp and the files around prover_state.h): per-device state (stream, MSM workspace,
// grow-only scratch buffers, NTT twiddle tables), evaluation domains, error
// reporting.  Definitions live in abi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/h2g.h"
#include "bn254.h"
#include "msm.h"
#include "ntt.h"

namespace h2g {
namespace rt {

extern thread_local std::string g_err;
extern std::recursive_mutex g_mu;

int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define HIPCHK(expr)                                                \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) return ::h2g::rt::hip_fail(_e, #expr);    \
  } while (0)

#define RCCHK(expr)         \
  do {                      \
    int _rc = (expr);       \
    if (_rc) return _rc;    \
  } while (0)

// Grow-only array of T in device memory (kPinned: in pinned host memory), owned by its
// holder: freed when the holder goes, and when a larger one replaces it.  ensure() is a
// compare on the warm path.  Growth waits for the device first -- kernels and copies in
// flight may still read the old allocation, and that they have finished must not rest on
// what hipFree happens to do -- so an address taken from `p` does not outlive the next
// ensure(): size first, then take pointers.
template <class T, bool kPinned = false>
struct DevArr {
  T* p = nullptr;
  size_t len = 0;
  DevArr() = default;
  DevArr(DevArr&& o) noexcept : p(o.p), len(o.len) { o.p = nullptr, o.len = 0; }
  DevArr& operator=(DevArr&& o) noexcept {
    std::swap(p, o.p);
    std::swap(len, o.len);
    return *this;
  }
  ~DevArr() { release(); }
  hipError_t ensure(size_t count) { return count <= len ? hipSuccess : grow(count); }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    len = 0;
  }
  template <class U>
  U* as() const { return reinterpret_cast<U*>(p); }

 private:
  hipError_t grow(size_t count) {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    release();
    e = kPinned ? hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault)
                : hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) len = count;
    else p = nullptr;
    return e;
  }
};
template <class T>
using PinArr = DevArr<T, true>;
using DevBuf = DevArr<uint8_t>;  // untyped scratch, sized in bytes

// A stream / an event that its holder owns: created on first use, destroyed with the holder
template <class H, hipError_t (*kDestroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
  Handle& operator=(Handle&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  ~Handle() {
    if (h) (void)kDestroy(h);
  }
  operator H() const { return h; }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  hipError_t ensure() { return h ? hipSuccess : hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t ensure() { return h ? hipSuccess : hipEventCreateWithFlags(&h, hipEventDisableTiming); }
};

struct NttKey {  // omega, and the scale folded into the first pass's twiddles (ntt.h NttTables::fold)
  int L;
  uint32_t w[8];
  uint32_t f[8];
  bool operator<(const NttKey& o) const {
    if (L != o.L) return L < o.L;
    const int c = std::memcmp(w, o.w, sizeof(w));
    if (c) return c < 0;
    return std::memcmp(f, o.f, sizeof(f)) < 0;
  }
};

// EvaluationDomain constants (halo2_backend/src/poly/domain.rs:38-144)
struct Domain {
  uint32_t j = 0, k = 0, ek = 0;
  Fr omega, omega_inv, ext_omega, ext_omega_inv, g_coset, g_coset_inv, ifft_div, ext_ifft_div, bary;
  std::vector<Fr> t_evals;
  DevArr<Fr> d_t;
};

struct Descriptor {
  int device = 0;
  void* d = nullptr;  // scalars (= mem.p), or bases (= window 0 of fb.table)
  size_t n = 0;
  bool is_base = false;
  DevBuf mem;         // the scalars, or bases too few for windows
  MsmFixedBase fb;    // fixed-base windows of resident bases (owned)
  Descriptor() = default;
  Descriptor(Descriptor&& o) noexcept
      : device(o.device), d(o.d), n(o.n), is_base(o.is_base), mem(std::move(o.mem)), fb(o.fb) {
    o.fb = MsmFixedBase{};
  }
  ~Descriptor() { msm_fixed_base_free(&fb); }
};

// Asynchronous fixed-base MSMs: whole MSMs on two streams with a workspace each, so that
// one MSM's latency-bound phases (partition tail, fixup, reduction) overlap another's
// accumulation.  (Pipelining by stage instead -- partitions, accumulations and reductions
// on three streams -- measured slower: a partition beside an accumulation gets CUs only
// as the accumulation's blocks retire; profiles/r03/s3/ab_msm_pipe.)  Results land in a
// pinned ring (one XYZZ point each): MSM_RING slots at first, and one more block of as many
// whenever a launch finds too few free (a stage launches all its commitments before it
// collects any, and may have any number of them).  Blocks are never moved or freed before
// shutdown, so an outstanding ticket's slot stays where it is.
static constexpr int MSM_STREAMS = 2;
static constexpr int MSM_RING = 64;
struct MsmTicket {
  int slot = -1;
  int ring = -1;
  int c = 0;
  hipEvent_t done = nullptr;
  int64_t shard_seq = -1;  // >= 0: the peers' slabs of this MSM are pending (h2g_shard_transport)
  bool remote = false;     // SPMD column ownership: another rank computes this MSM whole
};

struct Device {
  int id = 0;
  hipStream_t stream = nullptr;
  MsmWorkspace msm;
  DevBuf a, b, c, work, out;
  std::map<NttKey, NttTables> ntt_tables;
  void* h_windows = nullptr;  // pinned host copy of MSM window sums
  // async MSM slots
  MsmWorkspace mws[MSM_STREAMS];
  hipStream_t mstream[MSM_STREAMS] = {};
  int next_slot = 0;
  std::vector<void*> h_ring;        // pinned G1xyzz[MSM_RING] blocks: slot r is h_ring[r / MSM_RING][r % MSM_RING]
  std::vector<hipEvent_t> ring_ev;  // one per slot
  std::vector<char> ring_busy;
  int next_ring = 0;
  G1xyzz* ring_at(int r) const { return reinterpret_cast<G1xyzz*>(h_ring[(size_t)r / MSM_RING]) + r % MSM_RING; }
  // the prover's column-transform stream (prove_impl: xs) and its NTT work buffer -- an NTT
  // on it must not share `work` with the prover's stream
  hipStream_t xstream = nullptr;
  DevBuf xwork;
  hipEvent_t xev_in = nullptr, xev_done = nullptr;
  // the device pairing's line tables (pairing_dev.h PairingTable) of the verifier params last
  // used, keyed by the 32 words of (g2, s_g2); rebuilt on the host when the key changes
  DevBuf pair_tab;
  uint64_t pair_key[32] = {};
  bool pair_valid = false;
};

extern std::vector<std::unique_ptr<Device>> g_devs;
extern bool g_profile;
extern std::vector<MsmPhaseEvents> g_msm_prof;
extern int g_cur;
extern std::map<uint64_t, Descriptor> g_desc;
extern std::map<uint64_t, std::unique_ptr<Domain>> g_dom;
extern uint64_t g_next_handle;

Device* cur();
inline hipStream_t pick_stream(Device* d, void* s) { return s ? reinterpret_cast<hipStream_t>(s) : d->stream; }

Fr fr_from_limbs(const uint64_t* v);
void fr_to_limbs(const Fr& a, uint64_t* v);
Fr root_of_unity();
Fr zeta();
Fr fr_delta();
constexpr uint32_t FR_S = 28;

int domain_init(Domain* dm, uint32_t j, uint32_t k);  // host constants + device t-evaluations
Domain* get_dom(uint64_t h);  // null: no such handle (find_desc, and prover_state.h find_*, alike)
Descriptor* find_desc(uint64_t h);

int get_tables(Device* d, const Fr& omega, int L, hipStream_t st, NttTables* out, const Fr& fold = Fr::one());
int msm_dev_impl(Device* d, const void* sc, const void* bs, size_t n, int c, void* out, hipStream_t st);
int msm_host_impl(Device* d, const void* sc, const void* bs, size_t n, int c, uint64_t* out, int* is_id,
                  hipStream_t st);
int msm_fixed_host_impl(Device* d, const void* sc, const MsmFixedBase& fb, size_t off, size_t n, uint64_t* out,
                        int* is_id, hipStream_t st);
// launch sum_{i<n} sc[i] * bases[off+i] after the work already queued on `producer`
int msm_fixed_launch(Device* d, const void* sc, const MsmFixedBase& fb, size_t off, size_t n, hipStream_t producer,
                     MsmTicket* t);
// nb (<= MSM_MAX_BATCH) MSMs against the same windows as one batched pipeline; t[nb]
int msm_ring_init(Device* d);  // the asynchronous MSMs' streams, ring and events (once)
int msm_fixed_launch_batch(Device* d, const void* const* sc, int nb, const MsmFixedBase& fb, size_t off, size_t n,
                           hipStream_t producer, MsmTicket* t);
// wait for a launched MSM, affine result
int msm_collect(Device* d, MsmTicket* t, uint64_t* out_affine);
int msm_collect_xyzz(Device* d, MsmTicket* t, G1xyzz* out);
// make `consumer` wait until every launched MSM has finished reading its scalars
int msm_fence(Device* d, hipStream_t consumer);
int msm_desc_impl(Device* d, const void* sc, const Descriptor& ds, size_t off, size_t n, uint64_t* out, int* is_id,
                  hipStream_t st);
int ntt_dev_impl_batch(Device* d, const Fr* const* src, uint64_t n_in, Fr* const* dst, int count, uint64_t out_len,
                       int L, const Fr& omega, int in_dist, const Fr& iz1, const Fr& iz2, int has_scale,
                       const Fr& scale, int out_dist, const Fr& oz1, const Fr& oz2, hipStream_t st);
int ntt_dev_impl(Device* d, const Fr* src, uint64_t n_in, Fr* dst, uint64_t out_len, int L, const Fr& omega,
                 int in_dist, const Fr& iz1, const Fr& iz2, int has_scale, const Fr& scale, int out_dist,
                 const Fr& oz1, const Fr& oz2, hipStream_t st);

// EvaluationDomain maps on device pointers (domain.rs:216-316)
int lagrange_to_coeff(Device* d, const Domain& dm, const Fr* src, Fr* dst, hipStream_t st);
int coeff_to_extended(Device* d, const Domain& dm, const Fr* src, Fr* dst, hipStream_t st);
// `count` independent transforms, NTT_MAX_BATCH per launch (work buffer grows to match)
int lagrange_to_coeff_batch(Device* d, const Domain& dm, const Fr* const* src, Fr* const* dst, int count,
                            hipStream_t st);
int coeff_to_extended_batch(Device* d, const Domain& dm, const Fr* const* src, Fr* const* dst, int count,
                            hipStream_t st);
int extended_to_coeff(Device* d, const Domain& dm, const Fr* src, Fr* dst, hipStream_t st);
// sub-coset t (< 2^(ek - k)) of each polynomial's extended coset, n points each: the rows
// t + 2^(ek - k) m of coeff_to_extended, by an n-point transform with a fused input twist
int coeff_to_subcoset_batch(Device* d, const Domain& dm, const Fr* const* src, Fr* const* dst, int count, uint64_t t,
                            hipStream_t st);

}  // namespace rt
}  // namespace h2g
