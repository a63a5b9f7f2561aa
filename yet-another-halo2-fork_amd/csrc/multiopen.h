// multiopen.h -- the KZG multi-open argument on its own (internal: prover.cpp, verifier.cpp,
// kzg.cpp): ProverSHPLONK / ProverGWC::create_proof and the two verifiers' scalar assembly as
// functions over an explicit context, so that create_proof / verify_proof and the standalone
// entry points (h2g_multiopen_prove / _verify) run one SHPLONK and one GWC.
#pragma once
#include "prover_state.h"

namespace h2g {
namespace prv {

struct PolyRef {  // a committed polynomial in coefficient form (SHPLONK's "commitment identity")
  const Fr* p;
  uint64_t len;
};
struct OpenQ {  // ProverQuery: the polynomial's index stands for the reference's pointer equality
  int poly;
  Fr pt;
};

// What the prover side works on.  ProofRun fills it from the proving key's workspace;
// h2g_multiopen_prove from allocations of its own.
struct MultiopenCtx {
  Device* d = nullptr;
  const Params* prm = nullptr;
  hipStream_t st = nullptr;
  Transcript* tr = nullptr;
  size_t n = 0;  // the params' n: every scratch buffer below holds n Fr
  const std::vector<PolyRef>* polys = nullptr;
  const std::vector<OpenQ>* queries = nullptr;
  std::function<Fr(int, const Fr&)> ev;  // polys[i](pt), for every (i, pt) among the queries
  // device scratch: nx, hx, lx, q1 n Fr each; scr kate_scratch_len(n); small >= max(#points of a
  // rotation set, #GWC point groups) Fr
  Fr *nx = nullptr, *hx = nullptr, *lx = nullptr, *q1 = nullptr, *scr = nullptr, *small = nullptr;
  // GWC: one witness polynomial of n Fr per point group, grown on demand from `pool`
  std::vector<Fr*>* gwc_q = nullptr;
  Pool* pool = nullptr;
  // dst (device) <- src (host) on st; src stays valid until the stream is synchronised
  std::function<hipError_t(void*, const void*, size_t)> upload;
  std::function<void(const char*)> mark;  // stage clock (may be empty)
  // SPMD coefficient slabs (SHPLONK inside create_proof only): empty = {false, {0, n, n}, null}
  bool slabs = false;
  Slab sl;
  ProvingKey* slab_pk = nullptr;  // the slab buffers and the carries' evaluation scratch
};

int multiopen_shplonk(MultiopenCtx& c);
int multiopen_gwc(MultiopenCtx& c);

int fr_cmp(const Fr& a, const Fr& b);  // Ord on Fr: canonical numeric order

// ---- the verifier side: scalar assembly of the DualMSM (host only)
struct Term {
  uint32_t base;
  Fr s;
};
using Msm = std::vector<Term>;
void msm_merge(Msm& m);  // equal bases merged
constexpr uint32_t BASE_G1 = 0;  // the base index of the params' G1 generator

struct VerifierQ {  // VerifierQuery: a commitment (or MSM) key, a point index, the evaluation
  uint32_t key;
  int pt;  // index into MultiopenVerifyIo::point
  Fr eval;
};
struct MultiopenVerifyIo {
  Transcript* T = nullptr;
  std::vector<Fr> point;                  // the distinct opening points
  std::function<uint32_t()> read_point;   // TranscriptRead::read_point: the point's base index
  std::function<bool()> ok;               // false once a read failed
  std::function<void(Msm&, uint32_t, const Fr&)> add_obj;  // m += f * (the object behind `key`)
  long expect_groups = -1;  // GWC: the number of point groups the caller's layout has (-1: any)
};
enum { MULTIOPEN_SHPLONK = 0, MULTIOPEN_GWC = 1 };
// fills left / right; false: the argument is malformed
bool multiopen_verify_terms(int scheme, const std::vector<VerifierQ>& queries, MultiopenVerifyIo& io, Msm* left,
                            Msm* right);

// A proof that fails part-way leaves launched MSMs uncollected: their result ring entries
// would stay reserved.  Proofs run one at a time under the library lock and collect every
// MSM they launch, so on the way out the MSM streams are drained and the ring freed.
struct MsmRingGuard {
  Device* d;
  ~MsmRingGuard() {
    bool any = false;
    for (char b : d->ring_busy) any = any || b;
    if (!any) return;
    for (hipStream_t s : d->mstream)
      if (s) (void)hipStreamSynchronize(s);
    for (char& b : d->ring_busy) b = 0;
  }
};

// pk_serde.cpp: GroupEncoding::from_bytes of one G1 point on the host (the identity decodes
// to (0, 0); false: x >= p or no curve point)
bool g1_from_bytes_host(const uint8_t c[32], G1Affine* out);

// ---- transcript objects of the C ABI (h2g_transcript_*; kzg.cpp): TranscriptWrite / TranscriptRead
struct TranscriptObj {
  bool read = false;
  int kind = 0;
  std::vector<uint8_t> bytes;  // write mode: the bytes written; read mode: the proof
  size_t pos = 0;              // read mode: the next unread byte
  Transcript tr{nullptr, 0};   // its sink is `bytes` in write mode (rebind after a copy)
  TranscriptObj(bool rd, int k) : read(rd), kind(k), tr(rd ? nullptr : &bytes, k) {}
  TranscriptObj(const TranscriptObj& o) : read(o.read), kind(o.kind), bytes(o.bytes), pos(o.pos), tr(o.tr) {
    tr.set_sink(read ? nullptr : &bytes);
  }
  TranscriptObj& operator=(const TranscriptObj& o) {
    read = o.read, kind = o.kind, bytes = o.bytes, pos = o.pos, tr = o.tr;
    tr.set_sink(read ? nullptr : &bytes);
    return *this;
  }
  // TranscriptRead::read_point / read_scalar; false (state unchanged): the bytes end, the
  // encoding is invalid, or the point is the identity
  bool read_point(G1Affine* out);
  bool read_scalar(Fr* out);
};
extern std::map<uint64_t, std::unique_ptr<TranscriptObj>> g_transcripts;  // kzg.cpp
inline TranscriptObj* find_transcript(uint64_t h) { return find_handle(g_transcripts, h); }

}  // namespace prv
}  // namespace h2g
