// api_pipe.cpp — batches in host memory: the circuit's pool of per-device pipelines (HostPipe),
// the chunk ring and the sharding over devices.
#include <algorithm>
#include <cstring>
#include <thread>
#include "api_internal.hpp"

void pipe_free(HostPipe* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->st) (void)hipStreamSynchronize(p->st);
  if (p->cs) (void)hipStreamSynchronize(p->cs);
  delete p;
}
constexpr int kPoolIdleMax = 4;   // idle pipes kept per (circuit, device)

// a pipe of circuit c on `device` whose verifier holds `cap` proofs: an idle one of the pool (the
// smallest that fits), else a new one
int pipe_acquire(const p2v_circuit* c, int device, size_t cap, HostPipe** out) {
  *out = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->pool_mu);
    HostPipe* best = nullptr;
    for (HostPipe* p : c->pool)
      if (!p->busy && p->device == device && p->cap >= cap && (!best || p->cap < best->cap)) best = p;
    if (best) { best->busy = true; *out = best; return P2V_OK; }
  }
  auto* p = new HostPipe();
  p->device = device; p->cap = cap;
  int rc = P2V_OK;
  if (hipSetDevice(device) != hipSuccess || p->st.create() != hipSuccess || p->cs.create() != hipSuccess)
    rc = fail(P2V_E_DEVICE, "stream creation on device " + std::to_string(device));
  p2v_verifier* v = nullptr;
  if (rc == P2V_OK) rc = p2v_verifier_create(c, device, cap, &v);
  p->v.reset(v);
  if (rc != P2V_OK) { pipe_free(p); return rc; }
  p->busy = true;
  std::lock_guard<std::mutex> lk(c->pool_mu);
  c->pool.push_back(p);
  *out = p;
  return P2V_OK;
}

void pipe_release(const p2v_circuit* c, HostPipe* p, bool broken) {
  HostPipe* drop = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->pool_mu);
    p->busy = false;
    int idle = 0;
    for (HostPipe* q : c->pool) idle += (!q->busy && q->device == p->device) ? 1 : 0;
    if (broken || idle > kPoolIdleMax) {   // a pipe whose run failed is not reused
      c->pool.erase(std::remove(c->pool.begin(), c->pool.end(), p), c->pool.end());
      drop = p;
    }
  }
  pipe_free(drop);
}

// what a chunked call of n proofs of W words needs on pipe p: the ring (made once), the device
// statuses and their pinned copy, and for the binary path (want_ok) the same for the ok flags
int pipe_prepare(HostPipe* p, size_t n, size_t W, bool want_ok) {
  if (!p->have_ring) {
    for (int k = 0; k < HostPipe::kRing; k++) {
      HCK(p->ring[k].alloc(p->cap * W * 8));
      HCK(p->kring[k].alloc(p->cap * sizeof(uint32_t)));
      if (!p->copied[k]) HCK(p->copied[k].create());
      if (!p->freed[k]) HCK(p->freed[k].create());
    }
    p->have_ring = true;
  }
  HCK(p->dres.grow(n));
  if (want_ok) HCK(p->dok.grow(n));
  HCK(p->h_res.grow(n));
  if (want_ok) HCK(p->h_ok.grow(n));
  return P2V_OK;
}

// the verifier capacity for m proofs in chunks of ch: one chunk in 64-proof granules (powers of
// two), else the chunk
size_t pipe_cap(size_t m, size_t ch) {
  size_t cap = 64;
  while (cap < std::min(m, ch)) cap <<= 1;
  if (m > ch) cap = ch;
  return cap;
}

// verify m proofs (proof-major rows in host memory) on pipe p: one run for a single chunk (the
// latency path: H2D, kernels, D2H on the pipe's stream); otherwise chunks of <= p->cap proofs
// through the ring, copies on the copy stream, verification on the compute stream, statuses
// accumulated on the device and copied back once.  key_ids (host memory, or null: key 0): proof
// i's key, each chunk's slice copied with the chunk.
int pipe_run(HostPipe* p, const uint64_t* src, const uint32_t* key_ids, size_t m, int8_t* results, size_t W, size_t chunk) {
  HCK(hipSetDevice(p->device));
  if (m <= chunk) return p2v_verifier_run_keyed(p->v.get(), src, key_ids, m, results, nullptr, p->st, 0);
  RCK(pipe_prepare(p, m, W, false));
  const size_t nch = (m + chunk - 1) / chunk;
  for (size_t i = 0; i < nch; i++) {
    const int b = (int)(i % HostPipe::kRing);
    const size_t off = i * chunk, len = std::min(chunk, m - off);
    if (i >= (size_t)HostPipe::kRing) HCK(hipStreamWaitEvent(p->cs, p->freed[b], 0));   // its last reader is done
    HCK(hipMemcpyAsync(p->ring[b].p, src + off * W, len * W * 8, hipMemcpyHostToDevice, p->cs));
    if (key_ids) HCK(hipMemcpyAsync(p->kring[b].p, key_ids + off, len * sizeof(uint32_t), hipMemcpyHostToDevice, p->cs));
    HCK(hipEventRecord(p->copied[b], p->cs));
    HCK(hipStreamWaitEvent(p->st, p->copied[b], 0));
    RCK(p2v_verifier_run_keyed(p->v.get(), (const uint64_t*)p->ring[b].p, key_ids ? (const uint32_t*)p->kring[b].p : nullptr, len,
                               (int8_t*)p->dres.p + off, nullptr, p->st, P2V_FLAG_INPUT_DEVICE | P2V_FLAG_RESULT_DEVICE | P2V_FLAG_NO_SYNC));
    HCK(hipEventRecord(p->freed[b], p->st));
  }
  HCK(hipMemcpyAsync(p->h_res.p, p->dres.p, m, hipMemcpyDeviceToHost, p->st));
  HCK(hipStreamSynchronize(p->st));
  memcpy(results, p->h_res.p, m);
  return P2V_OK;
}

// the chunk size of a shard of m proofs: the given one, or (0) about an eighth of the shard in
// multiples of 256 between 256 and 16384, so a batch of a few thousand proofs still has several
// chunks in flight and a large one keeps its launches large
size_t auto_chunk(size_t m, size_t chunk) {
  if (chunk) return chunk;
  const size_t c = (m / 8 + 255) / 256 * 256;
  return std::min<size_t>(16384, std::max<size_t>(256, c));
}

extern "C" {

// p2v_verify_batch_devices and p2v_verify_batch_keyed: shards over `devices`, proof i against key
// key_ids[i] (null: key 0)
static int verify_batch_sharded(const p2v_circuit* c, const uint64_t* proofs, const uint32_t* key_ids, size_t n, int8_t* results,
                                const int* devices, int ndevices, size_t chunk) {
  if (!c || !devices || ndevices <= 0 || (n && (!proofs || !results))) return fail(P2V_E_ARG, "null argument / no devices");
  if (n == 0) return P2V_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device available: libp2v verifies on MI355X only (no CPU fallback)");
  for (int i = 0; i < ndevices; i++)
    if (devices[i] < 0 || devices[i] >= ndev) return fail(P2V_E_ARG, "bad device index " + std::to_string(devices[i]));
  const size_t W = (size_t)c->c.L.words;
  const int shards = (int)std::min<size_t>((size_t)ndevices, n);
  std::vector<int> rcs(shards, P2V_OK);
  std::vector<std::string> msgs(shards);
  auto work = [&](int s) {
    const size_t base = n / shards, extra = n % shards;   // p2v.shard_bounds
    const size_t a = s * base + std::min<size_t>(s, extra), b = a + base + ((size_t)s < extra ? 1 : 0);
    const size_t m = b - a;
    const size_t ch = m <= 64 ? m : auto_chunk(m, chunk);
    HostPipe* p = nullptr;
    int rc = pipe_acquire(c, devices[s], pipe_cap(m, ch), &p);
    if (rc == P2V_OK) {
      rc = pipe_run(p, proofs + a * W, key_ids ? key_ids + a : nullptr, m, results + a, W, ch);
      pipe_release(c, p, rc != P2V_OK);
    }
    if (rc != P2V_OK) msgs[s] = g_err;   // g_err is thread-local: carry the message back
    rcs[s] = rc;
  };
  if (shards == 1) work(0);   // the calling thread (a drop-in verifyProof call starts no thread)
  else {
    std::vector<std::thread> pool;
    for (int s = 0; s < shards; s++) pool.emplace_back(work, s);
    for (auto& t : pool) t.join();
  }
  for (int s = 0; s < shards; s++)
    if (rcs[s] != P2V_OK)
      return fail(rcs[s], "shard " + std::to_string(s) + " (device " + std::to_string(devices[s]) + "): " + msgs[s]);
  return P2V_OK;
}

int p2v_verify_batch_devices(const p2v_circuit* c, const uint64_t* proofs, size_t n, int8_t* results,
                             const int* devices, int ndevices, size_t chunk) {
  return verify_batch_sharded(c, proofs, nullptr, n, results, devices, ndevices, chunk);
}

int p2v_verify_batch_keyed(const p2v_circuit* c, const uint64_t* proofs, const uint32_t* key_ids, size_t n, int8_t* results, int device) {
  if (!c || (n && (!proofs || !results))) return fail(P2V_E_ARG, "null argument");
  return verify_batch_sharded(c, proofs, key_ids, n, results, &device, 1, 0);
}

int p2v_verify_batch(const p2v_circuit* c, const uint64_t* proofs, size_t n, int8_t* results, int device) {
  return p2v_verify_batch_keyed(c, proofs, nullptr, n, results, device);
}

}  // extern "C"
