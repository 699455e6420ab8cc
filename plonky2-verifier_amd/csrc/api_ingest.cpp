// api_ingest.cpp — JSON texts and plonky2 binary proofs packed on the device (json_pack.hip), the
// host readers for what the device packers do not take.
#include <algorithm>
#include <cstring>
#include <functional>
#include "api_internal.hpp"
#include "kernels.h"

extern "C" {

// ---- ingest: JSON texts or plonky2 binary proofs -> packed rows of v->in ----

// A batch's texts or bytes and its offsets (rebased to the batch's first byte) on the device, in
// j_blob / j_offs, with room for the packer's ok flags in j_ok.  rel is the offsets' host copy:
// the caller keeps it until the stream is synchronised.
static int stage_batch(p2v_verifier* v, const void* blob, const uint64_t* offsets, size_t n, std::vector<uint64_t>& rel, hipStream_t st) {
  const uint64_t base = offsets[0], bytes = offsets[n] - base;
  HCK(v->j_blob.grow(bytes + 64));   // + vector / unaligned-load slack
  HCK(v->j_offs.grow((n + 1) * 8));
  HCK(v->j_ok.grow(n));
  rel.resize(n + 1);
  for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
  HCK(hipMemcpyAsync(v->j_blob.p, (const uint8_t*)blob + base, bytes, hipMemcpyHostToDevice, st));
  HCK(hipMemcpyAsync(v->j_offs.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  return P2V_OK;
}

// the device packer's ok flags of the staged batch, read back through the pinned buffer
static int read_ok_flags(p2v_verifier* v, size_t n, std::vector<int8_t>& okf, hipStream_t st) {
  HCK(hipGetLastError());
  HCK(hipMemcpyAsync(v->h_res.p, v->j_ok.p, n, hipMemcpyDeviceToHost, st));
  HCK(hipStreamSynchronize(st));
  okf.assign(v->h_res.p, v->h_res.p + n);
  return P2V_OK;
}

// The proofs the device packer did not take (other formatting, exotic numbers, errors): the host
// reader, one row at a time.  pack_row(i, row) packs proof i or throws as p2v_pack_proof_json /
// _bytes do; codes[i] is that call's code.  n_device receives the count of device-packed proofs.
static int host_fallback(p2v_verifier* v, size_t n, const std::vector<int8_t>& okf, int32_t* codes, size_t* n_device,
                         hipStream_t st, const std::function<void(size_t, uint64_t*)>& pack_row) {
  const size_t W = (size_t)v->circ->c.L.words;
  std::vector<uint64_t> row(W);
  if (n_device) for (size_t i = 0; i < n; i++) *n_device += okf[i] ? 1 : 0;
  for (size_t i = 0; i < n; i++) {
    codes[i] = P2V_OK;
    if (okf[i]) continue;
    try {
      pack_row(i, row.data());
      HCK(hipMemcpyAsync((uint64_t*)v->in.p + i * W, row.data(), W * 8, hipMemcpyHostToDevice, st));
      HCK(hipStreamSynchronize(st));   // row is reused
    } catch (const ShapeError&) { codes[i] = P2V_E_SHAPE; }
    catch (...) { codes[i] = P2V_E_PARSE; }
  }
  return P2V_OK;
}

// h on the device in b, grown to bytes + slack
static hipError_t put(DevBuf& b, const void* h, size_t bytes, size_t slack) {
  hipError_t e = b.grow(bytes + slack);
  if (e == hipSuccess && bytes) e = hipMemcpy(b.p, h, bytes, hipMemcpyHostToDevice);
  return e;
}

// JSON texts: the device packer against the template, the host reader for the rest
static int pack_json_into(p2v_verifier* v, const char* blob, const uint64_t* offsets, size_t n,
                          int32_t* codes, size_t* n_device, void* stream_) {
  if (n_device) *n_device = 0;
  if (!v || (n && (!blob || !offsets || !codes))) return fail(P2V_E_ARG, "null argument");
  if (n > v->max_batch) return fail(P2V_E_ARG, "batch larger than max_batch");
  if (n == 0) return P2V_OK;
  HCK(hipSetDevice(v->device));
  HCK(input_buf(v));
  hipStream_t st = (hipStream_t)stream_;
  const Circuit& C = v->circ->c;
  const int64_t W = C.L.words;
  auto text = [&](size_t i) { return blob + offsets[i]; };
  auto tlen = [&](size_t i) { return (size_t)(offsets[i + 1] - offsets[i]); };
  std::vector<uint64_t> row((size_t)W);
  // template: keep the current one while it packs the batch's first proof, else rebuild it
  // from the first proof the full reader accepts
  bool fresh = false;
  if (!(v->have_tmpl && v->tmpl.pack(text(0), tlen(0), row.data()))) {
    v->have_tmpl = false;
    for (size_t i = 0; i < n && !v->have_tmpl && i < 64; i++) {
      try { v->have_tmpl = v->tmpl.build(C, text(i), tlen(i), row.data()); } catch (...) { v->have_tmpl = false; }
    }
    fresh = v->have_tmpl;
  }
  std::vector<uint8_t> skel; std::vector<int32_t> tok;
  const bool dev_ok = v->have_tmpl && (!fresh || v->tmpl.device_form(skel, tok));
  if (fresh && dev_ok) {
    HCK(put(v->j_skel, skel.data(), skel.size(), 64));   // + vector-load slack
    HCK(put(v->j_tok, tok.data(), tok.size() * sizeof(int32_t), 64));
    v->skel_len = (int64_t)skel.size(); v->ntok = (int64_t)tok.size();
  } else if (fresh || !v->have_tmpl) {
    // a new template without a device form (or none at all): drop the previous template's
    // device form, so no later batch pairs it with this host template
    v->skel_len = 0; v->ntok = 0;
  }
  std::vector<int8_t> okf(n, 0);
  std::vector<uint64_t> rel;
  if (dev_ok && v->ntok > 0) {
    RCK(stage_batch(v, blob, offsets, n, rel, st));
    k_json_pack<<<(unsigned)n, 256, 0, st>>>((const uint8_t*)v->j_blob.p, (const uint64_t*)v->j_offs.p, (int)n, (const uint8_t*)v->j_skel.p,
                                             v->skel_len, (const int32_t*)v->j_tok.p, v->ntok, (uint64_t*)v->in.p, W, (int8_t*)v->j_ok.p);
    RCK(read_ok_flags(v, n, okf, st));
  }
  return host_fallback(v, n, okf, codes, n_device, st, [&](size_t i, uint64_t* dst) {
    JVal pj = parse_json(text(i), tlen(i));
    pack_proof(C, pj, dst);
  });
}

// the circuit's byte map (circuit.cpp bytes_map) on the verifier's device, made once
static int ensure_bytes_map(p2v_verifier* v) {
  if (v->have_bmap) return P2V_OK;
  const BytesMap m = bytes_map(v->circ->c);
  HCK(put(v->b_rsrc, m.run_src.data(), m.run_src.size() * 8, 16));   // (a retry after a failure reuses what is there)
  HCK(put(v->b_rdst, m.run_dst.data(), m.run_dst.size() * 8, 16));
  HCK(put(v->b_rlen, m.run_len.data(), m.run_len.size() * 8, 16));
  HCK(put(v->b_coff, m.chk_off.data(), m.chk_off.size() * 8, 16));
  HCK(put(v->b_cval, m.chk_val.data(), m.chk_val.size(), 16));
  v->nruns = (int)m.run_len.size(); v->nchk = (int)m.chk_off.size(); v->bfixed = m.fixed;
  v->have_bmap = true;
  return P2V_OK;
}

// k_bytes_pack against v's byte map: n proofs of src (offsets offs) into rows, ok flags into ok
static void launch_bytes_pack(const p2v_verifier* v, const DevBuf& src, const DevBuf& offs, size_t n, void* rows, int8_t* ok, hipStream_t st) {
  const Circuit& C = v->circ->c;
  k_bytes_pack<<<(unsigned)n, 256, 0, st>>>((const uint8_t*)src.p, (const uint64_t*)offs.p, (int)n, (const int64_t*)v->b_rsrc.p,
                                            (const int64_t*)v->b_rdst.p, (const int64_t*)v->b_rlen.p, v->nruns, (const int64_t*)v->b_coff.p,
                                            (const uint8_t*)v->b_cval.p, v->nchk, v->bfixed, (int64_t)C.num_pis, C.L.pis,
                                            (uint64_t*)rows, C.L.words, ok);
}

// plonky2 binary proofs: k_bytes_pack against the circuit's byte map, the host reader for any
// proof that fails a check
static int pack_bytes_into(p2v_verifier* v, const uint8_t* blob, const uint64_t* offsets, size_t n,
                           int32_t* codes, size_t* n_device, void* stream_) {
  if (n_device) *n_device = 0;
  if (!v || (n && (!blob || !offsets || !codes))) return fail(P2V_E_ARG, "null argument");
  if (n > v->max_batch) return fail(P2V_E_ARG, "batch larger than max_batch");
  if (n == 0) return P2V_OK;
  HCK(hipSetDevice(v->device));
  HCK(input_buf(v));
  hipStream_t st = (hipStream_t)stream_;
  RCK(ensure_bytes_map(v));
  std::vector<int8_t> okf;
  std::vector<uint64_t> rel;
  RCK(stage_batch(v, blob, offsets, n, rel, st));
  launch_bytes_pack(v, v->j_blob, v->j_offs, n, v->in.p, (int8_t*)v->j_ok.p, st);
  RCK(read_ok_flags(v, n, okf, st));
  return host_fallback(v, n, okf, codes, n_device, st, [&](size_t i, uint64_t* dst) {
    pack_proof_bytes(v->circ->c, blob + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), dst);
  });
}

// plonky2 binary proofs in host memory, verified through the circuit's pooled pipe: per chunk the
// bytes are copied on the copy stream, packed on the device (k_bytes_pack into a ring slot) and
// verified on the compute stream, up to kRing chunks in flight.  Proofs the device packer flags
// are packed by the host reader afterwards and verified in one more run (or get the reader's
// code), so results and codes equal p2v_verifier_run_bytes'.
int p2v_verify_batch_bytes(const p2v_circuit* c, const uint8_t* blob, const uint64_t* offsets, size_t n,
                           int8_t* results, int32_t* codes, size_t* n_device, int device, size_t chunk) {
  if (n_device) *n_device = 0;
  if (!c || (n && (!blob || !offsets || !results || !codes))) return fail(P2V_E_ARG, "null argument");
  if (n == 0) return P2V_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device available: libp2v verifies on MI355X only (no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  const Circuit& C = c->c;
  const size_t W = (size_t)C.L.words;
  const size_t ch = auto_chunk(n, chunk);
  HostPipe* p = nullptr;
  int rc = pipe_acquire(c, device, pipe_cap(n, ch), &p);
  if (rc != P2V_OK) return rc;
  auto body = [&]() -> int {
    HCK(hipSetDevice(device));
    p2v_verifier* v = p->v.get();
    RCK(ensure_bytes_map(v));
    RCK(pipe_prepare(p, n, W, true));
    const size_t nch = (n + ch - 1) / ch;
    for (size_t i = 0; i < nch; i++) {
      const int b = (int)(i % HostPipe::kRing);
      const size_t off = i * ch, len = std::min(ch, n - off);
      const uint64_t base = offsets[off], bytes = offsets[off + len] - base;
      if (i >= (size_t)HostPipe::kRing) {
        HCK(hipEventSynchronize(p->copied[b]));              // the slot's host offsets are no longer read
        HCK(hipStreamWaitEvent(p->cs, p->freed[b], 0));      // its device buffers' last reader is done
      }
      HCK(p->bbytes[b].grow(bytes + 64));   // + unaligned-load slack
      HCK(p->boffs[b].grow((p->cap + 1) * 8));   // for the largest chunk (len <= cap): made once
      auto& ho = p->hoffs[b];
      ho.resize(len + 1);
      for (size_t k = 0; k <= len; k++) ho[k] = offsets[off + k] - base;
      HCK(hipMemcpyAsync(p->bbytes[b].p, blob + base, bytes, hipMemcpyHostToDevice, p->cs));
      HCK(hipMemcpyAsync(p->boffs[b].p, ho.data(), (len + 1) * 8, hipMemcpyHostToDevice, p->cs));
      HCK(hipEventRecord(p->copied[b], p->cs));
      HCK(hipStreamWaitEvent(p->st, p->copied[b], 0));
      launch_bytes_pack(v, p->bbytes[b], p->boffs[b], len, p->ring[b].p, (int8_t*)p->dok.p + off, p->st);
      HCK(hipGetLastError());
      RCK(p2v_verifier_run(v, (const uint64_t*)p->ring[b].p, len, (int8_t*)p->dres.p + off, nullptr, p->st,
                           P2V_FLAG_INPUT_DEVICE | P2V_FLAG_RESULT_DEVICE | P2V_FLAG_NO_SYNC));
      HCK(hipEventRecord(p->freed[b], p->st));
    }
    HCK(hipMemcpyAsync(p->h_res.p, p->dres.p, n, hipMemcpyDeviceToHost, p->st));
    HCK(hipMemcpyAsync(p->h_ok.p, p->dok.p, n, hipMemcpyDeviceToHost, p->st));
    HCK(hipStreamSynchronize(p->st));
    memcpy(results, p->h_res.p, n);
    // the proofs the device packer did not take: the host reader, then one more run for those it packs
    std::vector<size_t> redo;
    std::vector<uint64_t> rows;
    for (size_t i = 0; i < n; i++) {
      codes[i] = P2V_OK;
      if (p->h_ok.p[i]) { if (n_device) (*n_device)++; continue; }
      rows.resize((redo.size() + 1) * W);
      try {
        pack_proof_bytes(C, blob + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), rows.data() + redo.size() * W);
        redo.push_back(i);
      } catch (const ShapeError&) { codes[i] = P2V_E_SHAPE; results[i] = P2V_ERR_SHAPE; }
      catch (...) { codes[i] = P2V_E_PARSE; results[i] = P2V_ERR_PARSE; }
    }
    if (!redo.empty()) {
      std::vector<int8_t> rr(redo.size());
      RCK(pipe_run(p, rows.data(), nullptr, redo.size(), rr.data(), W, p->cap));
      for (size_t k = 0; k < redo.size(); k++) results[redo[k]] = rr[k];
    }
    return P2V_OK;
  };
  rc = body();
  pipe_release(c, p, rc != P2V_OK);
  return rc;
}

// the packed rows of v->in back to the host (words, if wanted), zeroed where a proof did not pack
static int finish_pack(p2v_verifier* v, int rc, size_t n, const int32_t* codes, uint64_t* words, void* stream_) {
  if (rc != P2V_OK || n == 0 || !words) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const size_t W = (size_t)v->circ->c.L.words;
  HCK(hipMemcpyAsync(words, v->in.p, n * W * 8, hipMemcpyDeviceToHost, st));
  HCK(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++)
    if (codes[i] != P2V_OK) memset(words + i * W, 0, W * 8);
  return P2V_OK;
}

// the packed rows of v->in verified; a proof that did not pack gets its reader's status
static int run_packed(p2v_verifier* v, int rc, size_t n, int8_t* results, const int32_t* codes, void* stream_) {
  if (rc != P2V_OK || n == 0) return rc;
  RCK(p2v_verifier_run(v, (const uint64_t*)v->in.p, n, results, nullptr, stream_, P2V_FLAG_INPUT_DEVICE));
  for (size_t i = 0; i < n; i++)
    if (codes[i] != P2V_OK) results[i] = codes[i] == P2V_E_SHAPE ? P2V_ERR_SHAPE : P2V_ERR_PARSE;
  return P2V_OK;
}

int p2v_verifier_pack_bytes(p2v_verifier* v, const uint8_t* blob, const uint64_t* offsets, size_t n,
                            int32_t* codes, size_t* n_device, uint64_t* words, void* stream_) {
  return finish_pack(v, pack_bytes_into(v, blob, offsets, n, codes, n_device, stream_), n, codes, words, stream_);
}

int p2v_verifier_run_bytes(p2v_verifier* v, const uint8_t* blob, const uint64_t* offsets, size_t n,
                           int8_t* results, int32_t* codes, size_t* n_device, void* stream_) {
  if (n && !results) return fail(P2V_E_ARG, "null argument");
  return run_packed(v, pack_bytes_into(v, blob, offsets, n, codes, n_device, stream_), n, results, codes, stream_);
}

int p2v_verifier_pack_json(p2v_verifier* v, const char* blob, const uint64_t* offsets, size_t n,
                           int32_t* codes, size_t* n_device, uint64_t* words, void* stream_) {
  return finish_pack(v, pack_json_into(v, blob, offsets, n, codes, n_device, stream_), n, codes, words, stream_);
}

int p2v_verifier_run_json(p2v_verifier* v, const char* blob, const uint64_t* offsets, size_t n,
                          int8_t* results, int32_t* codes, size_t* n_device, void* stream_) {
  if (n && !results) return fail(P2V_E_ARG, "null argument");
  return run_packed(v, pack_json_into(v, blob, offsets, n, codes, n_device, stream_), n, results, codes, stream_);
}

}  // extern "C"
