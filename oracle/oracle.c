/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C CPU restatement of the reference Haskell verifier (bkomuves/plonky2-verifier,
 * /root/reference/src) used as the parity checker for the HIP path.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it; the product
 * (libp2v) never links or calls it.
 *
 * Parity pinning: the reference cannot be built here (Haskell; no GHC, no cabal file —
 * see DESIGN.md §Oracle).  This restatement is pinned by the reference's only golden
 * vector, the Poseidon KAT (Hash/Poseidon.hs:27-35), by the Sage-recipe root-of-unity
 * identities (Algebra/Goldilocks.hs:58-67), by the commentary's permutation-count model
 * (commentary/FRI.md:248-265), and by accept/reject self-consistency on synthetic valid
 * proofs.  Everything beyond the KAT is "parity unpinned by the reference" in the sense
 * of the task statement; DESIGN.md records this.
 *
 * Structure follows the reference module by module; every function cites the file:line
 * it restates.  Semantics reproduced on purpose: inv(0) = 0,
 * lazy-duplex buffering, bit-reversed cosets, zip truncation, `error` ordering.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <setjmp.h>
#include "or_json.h"
#include "poseidon_constants.h"
#include "../include/p2v.h"

typedef uint64_t F;
typedef unsigned __int128 u128;
#define P_MOD 0xFFFFFFFF00000001ULL

/* ======================================================================= errors */
static __thread jmp_buf* g_jb;
static __thread char g_msg[512];
static __thread int g_code;

static void fail(int code, const char* msg) {
  g_code = code;
  snprintf(g_msg, sizeof g_msg, "%s", msg);
  longjmp(*g_jb, 1);
}

/* ======================================================================= arena */
typedef struct blk { struct blk* next; size_t used, cap; char data[]; } blk;
typedef struct { blk* head; } arena;
static void* aalloc(arena* a, size_t sz) {
  sz = (sz + 15) & ~(size_t)15;
  if (!a->head || a->head->used + sz > a->head->cap) {
    size_t cap = sz > (4u << 20) ? sz : (4u << 20);
    blk* b = (blk*)malloc(sizeof(blk) + cap);
    b->next = a->head; b->used = 0; b->cap = cap; a->head = b;
  }
  void* p = a->head->data + a->head->used; a->head->used += sz;
  memset(p, 0, sz);
  return p;
}
static void afree(arena* a) { blk* b = a->head; while (b) { blk* n = b->next; free(b); b = n; } a->head = NULL; }

/* ============================================================ Goldilocks field
 * Algebra/Goldilocks.hs:126-175 — canonical representatives, reduction mod p after
 * every operation; inv = pow x (p-2) so inv 0 = 0 (:155-156).                      */
static inline F fadd(F a, F b) { u128 s = (u128)a + b; if (s >= P_MOD) s -= P_MOD; return (F)s; }
static inline F fsub(F a, F b) { return a >= b ? a - b : (F)((u128)a + P_MOD - b); }
static inline F fneg(F a) { return a ? P_MOD - a : 0; }
static inline F fmul(F a, F b) { return (F)(((u128)a * b) % P_MOD); }
static F fpow(F x, u128 e) { F acc = 1, s = x; while (e) { if (e & 1) acc = fmul(acc, s); s = fmul(s, s); e >>= 1; } return acc; }
static inline F finv(F x) { return fpow(x, P_MOD - 2); }
static inline F fdiv(F a, F b) { return fmul(a, finv(b)); }
/* pow_ with negative exponent: pow (inv x) (-e)  (Goldilocks.hs:166-169) */
static F fpow_i(F x, long long e) { if (e == 0) return 1; if (e < 0) return fpow(finv(x), (u128)(-e)); return fpow(x, (u128)e); }
static const F MULT_GEN = 0xc65c18b67785d900ULL;      /* Goldilocks.hs:51-52 */
static const F TWO_ADIC_GEN = 0x64fdd1a46201e246ULL;  /* Goldilocks.hs:55-56 */

/* rootsOfUnity!k = h^(2^(32-k)), Goldilocks.hs:68-74 */
static F subgroup_gen(int k) {
  if (k < 0 || k > 32) fail(P2V_ERR_CIRCUIT, "subgroupGenerator: log2 out of range");
  F x = TWO_ADIC_GEN; for (int i = 0; i < 32 - k; i++) x = fmul(x, x); return x;
}

/* ================================================== quadratic extension F[X]/(X^2-7)
 * Algebra/GoldilocksExt.hs:54-100 */
typedef struct { F a, b; } E;
static inline E E0(void) { E r = {0, 0}; return r; }
static inline E Eb(F x) { E r = {x, 0}; return r; }           /* fromBase :31 */
static inline E Eadd(E x, E y) { E r = {fadd(x.a, y.a), fadd(x.b, y.b)}; return r; }
static inline E Esub(E x, E y) { E r = {fsub(x.a, y.a), fsub(x.b, y.b)}; return r; }
static inline E Eneg(E x) { E r = {fneg(x.a), fneg(x.b)}; return r; }
static inline E Emul(E x, E y) { E r = {fadd(fmul(x.a, y.a), fmul(7, fmul(x.b, y.b))), fadd(fmul(x.a, y.b), fmul(y.a, x.b))}; return r; }
static inline E Escale(F s, E x) { E r = {fmul(s, x.a), fmul(s, x.b)}; return r; }   /* scaleExt :70-71 */
static inline int Eeq(E x, E y) { return x.a == y.a && x.b == y.b; }
static E Einv(E x) {   /* invExt :76-80: recip of the norm, 0 -> 0 */
  F d = finv(fsub(fmul(x.a, x.a), fmul(7, fmul(x.b, x.b))));
  E r = {fmul(x.a, d), fmul(fneg(x.b), d)}; return r;
}
static inline E Ediv(E u, E v) { return Emul(u, Einv(v)); }
static E Epow(E x, long long e) {   /* powExt :90-100 */
  if (e == 0) return Eb(1);
  if (e < 0) { x = Einv(x); e = -e; }
  E acc = Eb(1), s = x;
  while (e) { if (e & 1) acc = Emul(acc, s); s = Emul(s, s); e >>= 1; }
  return acc;
}

/* "doubly extended" arithmetic: Ext over Expr evaluated in F^2 (Gate/Vars.hs:56-57,
 * GoldilocksExt.hs:54-61 instantiated at a = Expr; 7 is the literal LitE 7). */
typedef struct { E re, im; } EE;
static inline EE EEadd(EE x, EE y) { EE r = {Eadd(x.re, y.re), Eadd(x.im, y.im)}; return r; }
static inline EE EEsub(EE x, EE y) { EE r = {Esub(x.re, y.re), Esub(x.im, y.im)}; return r; }
static inline EE EEmul(EE x, EE y) {
  EE r = {Eadd(Emul(x.re, y.re), Emul(Eb(7), Emul(x.im, y.im))), Eadd(Emul(x.re, y.im), Emul(y.re, x.im))};
  return r;
}
static inline EE EEscale(E s, EE x) { EE r = {Emul(s, x.re), Emul(s, x.im)}; return r; }
static inline EE EEfromBase(E x) { EE r = {x, E0()}; return r; }

/* bit reversal, Algebra/FFT.hs:20-25 */
static uint64_t rev_bits(int n, uint64_t w) { uint64_t r = 0; for (int k = 0; k < n; k++) r |= ((w >> k) & 1) << (n - k - 1); return r; }

/* ================================================================ Poseidon
 * Hash/Poseidon.hs:42-101 (naive form, the one used for hashing) */
static F mds_coeff(int i, int j) { return OR_MDS_CIRC[(((j - i) % 12) + 12) % 12] + (i == j ? OR_MDS_DIAG[i] : 0); } /* Constants.hs:24-25 */
static F sbox1(F x) { return fpow(x, 7); }
static void linear_diffusion(F* s) {
  F t[12];
  for (int i = 0; i < 12; i++) { F acc = 0; for (int j = 0; j < 12; j++) acc = fadd(acc, fmul(mds_coeff(i, j), s[j])); t[i] = acc; }
  memcpy(s, t, sizeof t);
}
static void external_round(int r, F* s) { for (int i = 0; i < 12; i++) s[i] = sbox1(fadd(s[i], OR_ALL_ROUND_CONSTANTS[12 * r + i])); linear_diffusion(s); }
static void internal_round(int r, F* s) {
  s[0] = sbox1(fadd(s[0], OR_ALL_ROUND_CONSTANTS[12 * r]));
  for (int i = 1; i < 12; i++) s[i] = fadd(s[i], OR_ALL_ROUND_CONSTANTS[12 * r + i]);
  linear_diffusion(s);
}
static long long g_perm_count;   /* instrumentation for the commentary cost model */
void or_permutation(F* s) {
  g_perm_count++;
  for (int r = 0; r < 4; r++) external_round(r, s);
  for (int r = 4; r < 26; r++) internal_round(r, s);
  for (int r = 26; r < 30; r++) external_round(r, s);
}
long long or_perm_count(void) { return g_perm_count; }
void or_perm_count_reset(void) { g_perm_count = 0; }

/* sponge, Hash/Sponge.hs:26-31: overwrite mode, rate 8, no padding, [] -> zero digest */
static void sponge(const F* xs, long n, F out[4]) {
  F st[12] = {0};
  for (long i = 0; i < n; i += 8) {
    long k = n - i < 8 ? n - i : 8;
    for (long j = 0; j < k; j++) st[j] = xs[i + j];
    or_permutation(st);
  }
  memcpy(out, st, 4 * sizeof(F));
}
void or_sponge(const F* xs, long n, F* out) { sponge(xs, n, out); }

/* compress, Hash/Merkle.hs:21-23 */
static void compress(const F* x, const F* y, F out[4]) {
  F st[12] = {0};
  memcpy(st, x, 32); memcpy(st + 4, y, 32);
  or_permutation(st);
  memcpy(out, st, 32);
}

/* reconstructMerkleRoot / checkMerkleProof, Hash/Merkle.hs:27-42 */
static int check_merkle(const F (*cap)[4], int ncap, long idx, const F* leaf, long nleaf,
                        const F (*sib)[4], int nsib, int noop) {
  F cur[4];
  if (noop && nleaf <= 4) {   /* P2V_EXT_HASH_OR_NOOP: plonky2 hash_or_noop, the leaf zero-padded */
    memset(cur, 0, sizeof cur); memcpy(cur, leaf, (size_t)nleaf * sizeof(F));
  } else sponge(leaf, nleaf, cur);
  for (int k = 0; k < nsib; k++) {
    F nx[4];
    if ((idx & 1) == 0) compress(cur, sib[k], nx); else compress(sib[k], cur, nx);
    memcpy(cur, nx, 32); idx >>= 1;
  }
  if (idx < 0 || idx >= ncap) fail(P2V_ERR_SHAPE, "Prelude.!!: index too large (merkle cap)");
  return !memcmp(cap[idx], cur, 32);
}

/* =============================================================== data model
 * Types.hs:47-279 */
enum { G_ARITH, G_ARITH_EXT, G_BASESUM, G_COSET, G_CONST, G_EXP, G_LOOKUP, G_LOOKUPTABLE,
       G_MULEXT, G_NOOP, G_PI, G_POSEIDON, G_POSEIDON_MDS, G_RANDACC, G_REDUCING, G_REDUCING_EXT, G_UNKNOWN };
typedef struct { int kind; long long p0, p1, p2; F* weights; int nweights; } gate_t;   /* Gate/Base.hs:27-45 */

typedef struct {
  int num_wires, num_routed, num_const_cfg, r, max_qdf;
  int rate_bits, cap_height, pow_bits, nqueries;
  int strat;  /* 0 ConstantArityBits, 1 Fixed, 2 MinSize */
  int hiding; int* params_ar; int nparams_ar;   /* fri_params.hiding, .reduction_arity_bits (Types.hs:153-155) */
  unsigned ext;                                  /* P2V_EXT_* opt-in plonky2 conventions (include/p2v.h) */
  int strat_a, strat_b; int* fixed; int nfixed;
  int degree_bits;
  gate_t* gates; int ngates;
  int* sel_idx; int nsel_idx; int* grp_s; int* grp_e; int ngroups;
  int qdf, num_gate_constraints, num_constants, num_pis;
  F* k_is; int nk;
  int npp, nlp, nls;
  int nluts; int* lut_len; F** lut_in; F** lut_out;
  F (*cs_cap)[4]; int ncs_cap; F digest[4];
  arena mem;
} circuit_t;

typedef struct { F* leaf; int nleaf; F (*sib)[4]; int nsib; } eproof_t;
typedef struct { E* evals; int nevals; F (*sib)[4]; int nsib; } step_t;
typedef struct { eproof_t* init; int ninit; step_t* steps; int nsteps; } qround_t;
typedef struct {
  F* pis; int npis;
  F (*wires_cap)[4]; int nwc; F (*zs_cap)[4]; int nzc; F (*q_cap)[4]; int nqc;
  E *o_const, *o_sig, *o_wires, *o_zs, *o_zs_next, *o_pp, *o_quot, *o_lzs, *o_lzs_next;
  int n_const, n_sig, n_wires, n_zs, n_zs_next, n_pp, n_quot, n_lzs, n_lzs_next;
  F (**ccaps)[4]; int* nccap; int nccaps;
  qround_t* rounds; int nrounds;
  E* final_poly; int nfinal;
  F pow_witness;
  arena mem;
} proof_t;

/* ---------------------------------------------------------------- JSON decode */
static oj* req(const oj* o, const char* k) { oj* v = oj_get(o, k); if (!v) fail(P2V_ERR_PARSE, k); return v; }
static const oj* arr(const oj* o) { if (!o || o->kind != OJ_ARR) fail(P2V_ERR_PARSE, "expected array"); return o; }

/* Integer JSON -> F: aeson Integer then `mod p` (Goldilocks.hs:101-102) */
static F j_field(const oj* o) {
  if (!o || o->kind != OJ_NUM) fail(P2V_ERR_PARSE, "expected number");
  size_t i = 0; int neg = 0;
  if (o->text[0] == '-') { neg = 1; i = 1; }
  if (i >= o->len) fail(P2V_ERR_PARSE, "bad number");
  u128 acc = 0;
  for (; i < o->len; i++) {
    char c = o->text[i];
    if (c < '0' || c > '9') fail(P2V_ERR_PARSE, "non-integral number");
    acc = (acc * 10 + (unsigned)(c - '0')) % P_MOD;
  }
  return neg ? fneg((F)acc) : (F)acc;
}
static long long j_int(const oj* o) {
  if (!o || o->kind != OJ_NUM) fail(P2V_ERR_PARSE, "expected int");
  char buf[64]; size_t l = o->len < 63 ? o->len : 63; memcpy(buf, o->text, l); buf[l] = 0;
  for (size_t i = 0; i < l; i++) if (!((buf[i] >= '0' && buf[i] <= '9') || (i == 0 && buf[i] == '-'))) fail(P2V_ERR_PARSE, "non-integral int");
  return strtoll(buf, NULL, 10);
}
/* Word64 (LUT entries, Types.hs:30-35): must lie in [0, 2^64) then toF */
static F j_word64(const oj* o) {
  if (!o || o->kind != OJ_NUM || o->text[0] == '-') fail(P2V_ERR_PARSE, "expected Word64");
  u128 acc = 0;
  for (size_t i = 0; i < o->len; i++) {
    char c = o->text[i]; if (c < '0' || c > '9') fail(P2V_ERR_PARSE, "non-integral Word64");
    acc = acc * 10 + (unsigned)(c - '0'); if (acc >> 64) fail(P2V_ERR_PARSE, "Word64 out of range");
  }
  return (F)(acc % P_MOD);
}
static int j_bool(const oj* o) { if (!o || o->kind != OJ_BOOL) fail(P2V_ERR_PARSE, "expected bool"); return o->boolean; }

static void j_digest(const oj* o, F out[4]) {   /* Digest {"elements":[4]}  Hash/Digest.hs:40-44 */
  const oj* e = arr(req(o, "elements"));
  if (e->n != 4) fail(P2V_ERR_PARSE, "digest must have 4 elements");
  for (int i = 0; i < 4; i++) out[i] = j_field(e->items[i]);
}
static F (*j_cap(arena* m, const oj* o, int* n))[4] {   /* MerkleCap = [Digest] Types.hs:226-234 */
  const oj* a = arr(o); *n = (int)a->n;
  F (*c)[4] = (F (*)[4])aalloc(m, (a->n + 1) * 32);
  for (size_t i = 0; i < a->n; i++) j_digest(a->items[i], c[i]);
  return c;
}
static F* j_fields(arena* m, const oj* o, int* n) {
  const oj* a = arr(o); *n = (int)a->n;
  F* v = (F*)aalloc(m, (a->n + 1) * 8);
  for (size_t i = 0; i < a->n; i++) v[i] = j_field(a->items[i]);
  return v;
}
static E* j_exts(arena* m, const oj* o, int* n) {   /* Ext JSON = [a,b] GoldilocksExt.hs:46-50 */
  const oj* a = arr(o); *n = (int)a->n;
  E* v = (E*)aalloc(m, (a->n + 1) * sizeof(E));
  for (size_t i = 0; i < a->n; i++) {
    const oj* t = arr(a->items[i]); if (t->n != 2) fail(P2V_ERR_PARSE, "ext must be a pair");
    v[i].a = j_field(t->items[0]); v[i].b = j_field(t->items[1]);
  }
  return v;
}

/* ---------------------------------------------------------------- gate strings
 * Gate/Parser.hs:27-242 — a hand-rolled restatement of the Parsec grammar.  Every
 * alternative is wrapped in `try`, so each is attempted from the start of the string. */
typedef struct { const char* s; } GP;
static void g_spaces(GP* p) { while (*p->s == ' ' || *p->s == '\t' || *p->s == '\n' || *p->s == '\r' || *p->s == '\f' || *p->s == '\v') p->s++; }
static int g_str(GP* p, const char* lit) { size_t l = strlen(lit); if (strncmp(p->s, lit, l)) return 0; p->s += l; return 1; }
static int g_char(GP* p, char c) { if (*p->s != c) return 0; p->s++; return 1; }
static int g_integer(GP* p, long long* out, F* fout) {   /* many1 digit, read */
  if (*p->s < '0' || *p->s > '9') return 0;
  unsigned long long w = 0; u128 m = 0;
  while (*p->s >= '0' && *p->s <= '9') { unsigned d = (unsigned)(*p->s - '0'); w = w * 10 + d; m = (m * 10 + d) % P_MOD; p->s++; }
  if (out) *out = (long long)w;   /* fromInteger :: Integer -> Int wraps mod 2^64 */
  if (fout) *fout = (F)m;
  return 1;
}
static int g_comma(GP* p) { if (!g_char(p, ',')) return 0; g_spaces(p); return 1; }
static int g_kv_int(GP* p, const char* key, long long* v) {
  if (!g_str(p, key)) return 0; g_spaces(p); if (!g_char(p, ':')) return 0; g_spaces(p);
  if (!g_integer(p, v, NULL)) return 0; g_spaces(p); return 1;
}
static int g_list(GP* p, arena* m, F** out, int* n, int bytes) {
  if (!g_char(p, '[')) return 0; g_spaces(p);
  int cap = 16, k = 0; F* buf = (F*)malloc(cap * sizeof(F));
  F v; long long iv;
  if (g_integer(p, &iv, &v)) {
    buf[k++] = bytes ? (F)(uint8_t)iv : v;
    while (*p->s == ',') {
      GP save = *p; g_comma(p);
      if (!g_integer(p, &iv, &v)) { *p = save; free(buf); return 0; }   /* sepBy: sep consumed, p failed */
      if (k == cap) { cap *= 2; buf = (F*)realloc(buf, cap * sizeof(F)); }
      buf[k++] = bytes ? (F)(uint8_t)iv : v;
    }
  }
  if (!g_char(p, ']')) { free(buf); return 0; }
  g_spaces(p);
  if (m) { *out = (F*)aalloc(m, (k + 1) * sizeof(F)); memcpy(*out, buf, k * sizeof(F)); *n = k; }
  free(buf); return 1;
}
static int g_kv_list(GP* p, const char* key, arena* m, F** out, int* n, int bytes) {
  if (!g_str(p, key)) return 0; g_spaces(p); if (!g_char(p, ':')) return 0; g_spaces(p);
  if (!g_list(p, m, out, n, bytes)) return 0; g_spaces(p); return 1;
}
static int g_open(GP* p, const char* name) { if (!g_str(p, name)) return 0; g_spaces(p); if (!g_char(p, '{')) return 0; g_spaces(p); return 1; }
static int g_close(GP* p) { g_spaces(p); if (!g_char(p, '}')) return 0; g_spaces(p); return 1; }
static const char* PHANTOM = "_phantom: PhantomData<plonky2_field::goldilocks_field::GoldilocksField>";

static gate_t parse_gate(const char* str, arena* m) {
  gate_t g; memset(&g, 0, sizeof g);
  GP p; long long a, b, c; F* lst; int nl;
  /* ArithmeticGate (withEOF) */
  p.s = str; if (g_open(&p, "ArithmeticGate") && g_kv_int(&p, "num_ops", &a) && g_close(&p) && !*p.s) { g.kind = G_ARITH; g.p0 = a; return g; }
  p.s = str; if (g_open(&p, "ArithmeticExtensionGate") && g_kv_int(&p, "num_ops", &a) && g_close(&p) && !*p.s) { g.kind = G_ARITH_EXT; g.p0 = a; return g; }
  p.s = str; if (g_open(&p, "BaseSumGate") && g_kv_int(&p, "num_limbs", &a) && g_close(&p) && g_char(&p, '+')) {
    g_spaces(&p); if (g_kv_int(&p, "Base", &b) && !*p.s) { g.kind = G_BASESUM; g.p0 = a; g.p1 = b; return g; } }
  p.s = str; if (g_open(&p, "CosetInterpolationGate") && g_kv_int(&p, "subgroup_bits", &a) && g_comma(&p) &&
                 g_kv_int(&p, "degree", &b) && g_comma(&p) && g_kv_list(&p, "barycentric_weights", m, &lst, &nl, 0) &&
                 g_comma(&p) && g_str(&p, PHANTOM)) {
    g_spaces(&p); if (g_close(&p) && g_str(&p, "<D=2>") && !*p.s) { g.kind = G_COSET; g.p0 = a; g.p1 = b; g.weights = lst; g.nweights = nl; return g; } }
  p.s = str; if (g_open(&p, "ConstantGate") && g_kv_int(&p, "num_consts", &a) && g_close(&p)) { g.kind = G_CONST; g.p0 = a; return g; }
  p.s = str; if (g_open(&p, "ExponentiationGate") && g_kv_int(&p, "num_power_bits", &a) && g_close(&p)) { g.kind = G_EXP; g.p0 = a; return g; }
  p.s = str; if (g_open(&p, "LookupGate") && g_kv_int(&p, "num_slots", &a) && g_comma(&p) && g_kv_list(&p, "lut_hash", NULL, NULL, NULL, 1) && g_close(&p)) { g.kind = G_LOOKUP; g.p0 = a; return g; }
  p.s = str; if (g_open(&p, "LookupTableGate") && g_kv_int(&p, "num_slots", &a) && g_comma(&p) && g_kv_list(&p, "lut_hash", NULL, NULL, NULL, 1) &&
                 g_comma(&p) && g_kv_int(&p, "last_lut_row", &c) && g_close(&p)) { g.kind = G_LOOKUPTABLE; g.p0 = a; g.p2 = c; return g; }
  p.s = str; if (g_open(&p, "MulExtensionGate") && g_kv_int(&p, "num_ops", &a) && g_close(&p)) { g.kind = G_MULEXT; g.p0 = a; return g; }
  p.s = str; if (g_str(&p, "NoopGate")) { g.kind = G_NOOP; return g; }
  p.s = str; if (g_str(&p, "PublicInputGate")) { g.kind = G_PI; return g; }
  p.s = str; if (g_str(&p, "PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=") && g_integer(&p, &a, NULL) && g_char(&p, '>') && !*p.s) { g.kind = G_POSEIDON; g.p0 = a; return g; }
  p.s = str; if (g_str(&p, "PoseidonMdsGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=") && g_integer(&p, &a, NULL) && g_char(&p, '>') && !*p.s) { g.kind = G_POSEIDON_MDS; g.p0 = a; return g; }
  p.s = str; if (g_open(&p, "RandomAccessGate") && g_kv_int(&p, "bits", &a) && g_comma(&p) && g_kv_int(&p, "num_copies", &b) && g_comma(&p) &&
                 g_kv_int(&p, "num_extra_constants", &c) && g_comma(&p) && g_str(&p, PHANTOM)) {
    g_spaces(&p); if (g_close(&p) && g_str(&p, "<D=2>")) { g.kind = G_RANDACC; g.p0 = a; g.p1 = b; g.p2 = c; return g; } }
  p.s = str; if (g_open(&p, "ReducingGate") && g_kv_int(&p, "num_coeffs", &a)) { g_str(&p, "<D=2>"); if (g_close(&p)) { g.kind = G_REDUCING; g.p0 = a; return g; } }
  p.s = str; if (g_open(&p, "ReducingExtensionGate") && g_kv_int(&p, "num_coeffs", &a)) { g_str(&p, "<D=2>"); if (g_close(&p)) { g.kind = G_REDUCING_EXT; g.p0 = a; return g; } }
  g.kind = G_UNKNOWN; return g;
}

/* --------------------------------------------------------------- circuit load */
static void load_circuit(circuit_t* C, const oj* common, const oj* vkey) {
  arena* m = &C->mem;
  const oj* cfg = req(common, "config");
  C->num_wires = (int)j_int(req(cfg, "num_wires"));
  C->num_routed = (int)j_int(req(cfg, "num_routed_wires"));
  C->num_const_cfg = (int)j_int(req(cfg, "num_constants"));
  (void)j_bool(req(cfg, "use_base_arithmetic_gate"));
  (void)j_int(req(cfg, "security_bits"));
  C->r = (int)j_int(req(cfg, "num_challenges"));
  (void)j_bool(req(cfg, "zero_knowledge"));
  (void)j_bool(req(cfg, "randomize_unused_wires"));
  C->max_qdf = (int)j_int(req(cfg, "max_quotient_degree_factor"));
  const oj* fc = req(cfg, "fri_config");
  C->rate_bits = (int)j_int(req(fc, "rate_bits"));
  C->cap_height = (int)j_int(req(fc, "cap_height"));
  C->pow_bits = (int)j_int(req(fc, "proof_of_work_bits"));
  C->nqueries = (int)j_int(req(fc, "num_query_rounds"));
  const oj* rs = req(fc, "reduction_strategy");   /* Types.hs:134-143 */
  if (rs->kind != OJ_OBJ || rs->n != 1) fail(P2V_ERR_PARSE, "reduction_strategy: expecting a singleton object");
  if (!strcmp(rs->keys[0], "ConstantArityBits")) {
    const oj* ab = arr(rs->items[0]); if (ab->n != 2) fail(P2V_ERR_PARSE, "ConstantArityBits");
    C->strat = 0; C->strat_a = (int)j_int(ab->items[0]); C->strat_b = (int)j_int(ab->items[1]);
  } else if (!strcmp(rs->keys[0], "Fixed")) {
    const oj* fx = arr(rs->items[0]); C->strat = 1; C->nfixed = (int)fx->n;
    C->fixed = (int*)aalloc(m, (fx->n + 1) * sizeof(int));
    for (size_t i = 0; i < fx->n; i++) C->fixed[i] = (int)j_int(fx->items[i]);
  } else if (!strcmp(rs->keys[0], "MinSize")) {   /* Maybe Log2: null or a number */
    C->strat = 2;
    if (rs->items[0]->kind != OJ_NULL) (void)j_int(rs->items[0]);
  }
  else fail(P2V_ERR_PARSE, "unrecognized FRI reduction strategy");
  const oj* fp = req(common, "fri_params");
  C->hiding = j_bool(req(fp, "hiding"));
  C->degree_bits = (int)j_int(req(fp, "degree_bits"));
  {
    const oj* ra = arr(req(fp, "reduction_arity_bits"));
    C->nparams_ar = (int)ra->n; C->params_ar = (int*)aalloc(m, (ra->n + 1) * sizeof(int));
    for (size_t i = 0; i < ra->n; i++) C->params_ar[i] = (int)j_int(ra->items[i]);
  }
  (void)req(fp, "config");
  const oj* gs = arr(req(common, "gates"));
  C->ngates = (int)gs->n; C->gates = (gate_t*)aalloc(m, (gs->n + 1) * sizeof(gate_t));
  for (size_t i = 0; i < gs->n; i++) {
    if (gs->items[i]->kind != OJ_STR) fail(P2V_ERR_PARSE, "gate must be a string");
    C->gates[i] = parse_gate(gs->items[i]->text, m);
  }
  const oj* si = req(common, "selectors_info");
  const oj* sidx = arr(req(si, "selector_indices"));
  C->nsel_idx = (int)sidx->n; C->sel_idx = (int*)aalloc(m, (sidx->n + 1) * sizeof(int));
  for (size_t i = 0; i < sidx->n; i++) C->sel_idx[i] = (int)j_int(sidx->items[i]);
  const oj* grps = arr(req(si, "groups"));
  C->ngroups = (int)grps->n; C->grp_s = (int*)aalloc(m, (grps->n + 1) * sizeof(int)); C->grp_e = (int*)aalloc(m, (grps->n + 1) * sizeof(int));
  for (size_t i = 0; i < grps->n; i++) { C->grp_s[i] = (int)j_int(req(grps->items[i], "start")); C->grp_e[i] = (int)j_int(req(grps->items[i], "end")); }
  C->qdf = (int)j_int(req(common, "quotient_degree_factor"));
  C->num_gate_constraints = (int)j_int(req(common, "num_gate_constraints"));
  C->num_constants = (int)j_int(req(common, "num_constants"));
  C->num_pis = (int)j_int(req(common, "num_public_inputs"));
  C->k_is = j_fields(m, req(common, "k_is"), &C->nk);
  C->npp = (int)j_int(req(common, "num_partial_products"));
  C->nlp = (int)j_int(req(common, "num_lookup_polys"));
  C->nls = (int)j_int(req(common, "num_lookup_selectors"));
  const oj* luts = arr(req(common, "luts"));
  C->nluts = (int)luts->n;
  C->lut_len = (int*)aalloc(m, (luts->n + 1) * sizeof(int));
  C->lut_in = (F**)aalloc(m, (luts->n + 1) * sizeof(F*)); C->lut_out = (F**)aalloc(m, (luts->n + 1) * sizeof(F*));
  for (size_t t = 0; t < luts->n; t++) {
    const oj* L = arr(luts->items[t]); C->lut_len[t] = (int)L->n;
    C->lut_in[t] = (F*)aalloc(m, (L->n + 1) * 8); C->lut_out[t] = (F*)aalloc(m, (L->n + 1) * 8);
    for (size_t i = 0; i < L->n; i++) {
      const oj* pr = arr(L->items[i]); if (pr->n != 2) fail(P2V_ERR_PARSE, "lut entry must be a pair");
      C->lut_in[t][i] = j_word64(pr->items[0]); C->lut_out[t][i] = j_word64(pr->items[1]);
    }
  }
  C->cs_cap = j_cap(m, req(vkey, "constants_sigmas_cap"), &C->ncs_cap);   /* Types.hs:236-240 */
  j_digest(req(vkey, "circuit_digest"), C->digest);
}

static void load_proof(proof_t* P, const oj* root) {
  arena* m = &P->mem;
  const oj* pr = req(root, "proof");
  P->pis = j_fields(m, req(root, "public_inputs"), &P->npis);
  P->wires_cap = j_cap(m, req(pr, "wires_cap"), &P->nwc);
  P->zs_cap = j_cap(m, req(pr, "plonk_zs_partial_products_cap"), &P->nzc);
  P->q_cap = j_cap(m, req(pr, "quotient_polys_cap"), &P->nqc);
  const oj* o = req(pr, "openings");   /* OpeningSet, drop 8 — Types.hs:265-279 */
  P->o_const = j_exts(m, req(o, "constants"), &P->n_const);
  P->o_sig = j_exts(m, req(o, "plonk_sigmas"), &P->n_sig);
  P->o_wires = j_exts(m, req(o, "wires"), &P->n_wires);
  P->o_zs = j_exts(m, req(o, "plonk_zs"), &P->n_zs);
  P->o_zs_next = j_exts(m, req(o, "plonk_zs_next"), &P->n_zs_next);
  P->o_pp = j_exts(m, req(o, "partial_products"), &P->n_pp);
  P->o_quot = j_exts(m, req(o, "quotient_polys"), &P->n_quot);
  P->o_lzs = j_exts(m, req(o, "lookup_zs"), &P->n_lzs);
  P->o_lzs_next = j_exts(m, req(o, "lookup_zs_next"), &P->n_lzs_next);
  const oj* fp = req(pr, "opening_proof");   /* FriProof drop 4 — Types.hs:176-185 */
  const oj* cc = arr(req(fp, "commit_phase_merkle_caps"));
  P->nccaps = (int)cc->n;
  P->ccaps = (F (**)[4])aalloc(m, (cc->n + 1) * sizeof(void*)); P->nccap = (int*)aalloc(m, (cc->n + 1) * sizeof(int));
  for (size_t i = 0; i < cc->n; i++) P->ccaps[i] = j_cap(m, cc->items[i], &P->nccap[i]);
  const oj* qr = arr(req(fp, "query_round_proofs"));
  P->nrounds = (int)qr->n; P->rounds = (qround_t*)aalloc(m, (qr->n + 1) * sizeof(qround_t));
  for (size_t q = 0; q < qr->n; q++) {
    const oj* it = req(req(qr->items[q], "initial_trees_proof"), "evals_proofs");
    const oj* ita = arr(it);
    qround_t* R = &P->rounds[q];
    R->ninit = (int)ita->n; R->init = (eproof_t*)aalloc(m, (ita->n + 1) * sizeof(eproof_t));
    for (size_t t = 0; t < ita->n; t++) {
      const oj* pair = arr(ita->items[t]); if (pair->n != 2) fail(P2V_ERR_PARSE, "evals_proofs entry must be a pair");
      R->init[t].leaf = j_fields(m, pair->items[0], &R->init[t].nleaf);
      R->init[t].sib = j_cap(m, req(pair->items[1], "siblings"), &R->init[t].nsib);
    }
    const oj* st = arr(req(qr->items[q], "steps"));
    R->nsteps = (int)st->n; R->steps = (step_t*)aalloc(m, (st->n + 1) * sizeof(step_t));
    for (size_t s = 0; s < st->n; s++) {
      R->steps[s].evals = j_exts(m, req(st->items[s], "evals"), &R->steps[s].nevals);
      R->steps[s].sib = j_cap(m, req(req(st->items[s], "merkle_proof"), "siblings"), &R->steps[s].nsib);
    }
  }
  P->final_poly = j_exts(m, req(req(fp, "final_poly"), "coeffs"), &P->nfinal);
  P->pow_witness = j_field(req(fp, "pow_witness"));
}

/* ================================================================ duplex
 * Challenge/Pure.hs:27-107 — literal state machine with the lazy input buffer. */
typedef struct { F st[12]; int absorbing; F buf[8]; int nbuf; F out[8]; int nout, outpos; } duplex_t;
static void dx_init(duplex_t* d) { memset(d, 0, sizeof *d); d->absorbing = 1; }
static void dx_duplex(duplex_t* d) {   /* duplex inp old = permutation (overwrite inp old) :38-39 */
  for (int i = 0; i < d->nbuf; i++) d->st[i] = d->buf[i];
  or_permutation(d->st);
}
static void dx_fresh(duplex_t* d) {   /* freshSqueezing: out = reverse (take 8 state) :41-46 */
  d->absorbing = 0; for (int i = 0; i < 8; i++) d->out[i] = d->st[7 - i]; d->nout = 8; d->outpos = 0;
}
static void dx_absorb(duplex_t* d, F x) {   /* absorbFelt :50-58 */
  if (!d->absorbing) { d->absorbing = 1; d->nbuf = 0; }
  if (d->nbuf < 8) { d->buf[d->nbuf++] = x; return; }
  dx_duplex(d); d->nbuf = 0; d->buf[d->nbuf++] = x;
}
static F dx_squeeze(duplex_t* d) {   /* squeezeFelt :60-69 */
  if (d->absorbing) { dx_duplex(d); d->nbuf = 0; dx_fresh(d); }   /* empty inp: duplex [] old = permutation old */
  else if (d->outpos == d->nout) { or_permutation(d->st); dx_fresh(d); }
  return d->out[d->outpos++];
}
static void dx_absorb_n(duplex_t* d, const F* xs, long n) { for (long i = 0; i < n; i++) dx_absorb(d, xs[i]); }
static void dx_absorb_cap(duplex_t* d, const F (*cap)[4], int n) { for (int i = 0; i < n; i++) dx_absorb_n(d, cap[i], 4); }
static void dx_absorb_exts(duplex_t* d, const E* v, int n) { for (int i = 0; i < n; i++) { dx_absorb(d, v[i].a); dx_absorb(d, v[i].b); } }
static E dx_squeeze_ext(duplex_t* d) { E r; r.a = dx_squeeze(d); r.b = dx_squeeze(d); return r; }

/* ============================================================ challenges
 * Challenge/Verifier.hs:45-103, Challenge/FRI.hs:24-104 */
typedef struct { F A, B, alpha, delta; } ldelta_t;
typedef struct {
  F pi_hash[4];
  F *betas, *gammas, *alphas; ldelta_t* deltas; int ndeltas;
  E zeta;
  E fri_alpha; E* fri_betas; int nfri_betas; F pow_response; long* query_idx; int nquery;
  int unit_filters;   /* parity mode (or_verify full_trace bit 1): gate filters and lookup selectors := 1 */
} chal_t;

/* toFriOpenings, Challenge/FRI.hs:46-61 */
static E* fri_batch_this(arena* m, const proof_t* P, int* n) {
  *n = P->n_const + P->n_sig + P->n_wires + P->n_zs + P->n_pp + P->n_quot + P->n_lzs;
  E* v = (E*)aalloc(m, (*n + 1) * sizeof(E)); int k = 0;
  memcpy(v + k, P->o_const, P->n_const * sizeof(E)); k += P->n_const;
  memcpy(v + k, P->o_sig, P->n_sig * sizeof(E)); k += P->n_sig;
  memcpy(v + k, P->o_wires, P->n_wires * sizeof(E)); k += P->n_wires;
  memcpy(v + k, P->o_zs, P->n_zs * sizeof(E)); k += P->n_zs;
  memcpy(v + k, P->o_pp, P->n_pp * sizeof(E)); k += P->n_pp;
  memcpy(v + k, P->o_quot, P->n_quot * sizeof(E)); k += P->n_quot;
  memcpy(v + k, P->o_lzs, P->n_lzs * sizeof(E)); k += P->n_lzs;
  return v;
}
static E* fri_batch_next(arena* m, const proof_t* P, int* n) {
  *n = P->n_zs_next + P->n_lzs_next;
  E* v = (E*)aalloc(m, (*n + 1) * sizeof(E));
  memcpy(v, P->o_zs_next, P->n_zs_next * sizeof(E));
  memcpy(v + P->n_zs_next, P->o_lzs_next, P->n_lzs_next * sizeof(E));
  return v;
}

static void proof_challenges(arena* m, const circuit_t* C, const proof_t* P, chal_t* ch) {
  int r = C->r;
  duplex_t d; dx_init(&d);
  sponge(P->pis, P->npis, ch->pi_hash);
  dx_absorb_n(&d, C->digest, 4);
  dx_absorb_n(&d, ch->pi_hash, 4);
  dx_absorb_cap(&d, (const F (*)[4])P->wires_cap, P->nwc);
  ch->betas = (F*)aalloc(m, (r + 1) * 8); ch->gammas = (F*)aalloc(m, (r + 1) * 8); ch->alphas = (F*)aalloc(m, (r + 1) * 8);
  for (int i = 0; i < r; i++) ch->betas[i] = dx_squeeze(&d);
  for (int i = 0; i < r; i++) ch->gammas[i] = dx_squeeze(&d);
  if (C->nlp > 0) {   /* has_lookup :66 — mkLookupDeltaList (betas ++ gammas ++ deltas) :36-40,82-86 */
    F* all = (F*)aalloc(m, (4 * r + 1) * 8);
    for (int i = 0; i < r; i++) { all[i] = ch->betas[i]; all[r + i] = ch->gammas[i]; }
    for (int i = 0; i < 2 * r; i++) all[2 * r + i] = dx_squeeze(&d);
    ch->ndeltas = r; ch->deltas = (ldelta_t*)aalloc(m, (r + 1) * sizeof(ldelta_t));
    for (int i = 0; i < r; i++) { ch->deltas[i].A = all[4 * i]; ch->deltas[i].B = all[4 * i + 1]; ch->deltas[i].alpha = all[4 * i + 2]; ch->deltas[i].delta = all[4 * i + 3]; }
  }
  dx_absorb_cap(&d, (const F (*)[4])P->zs_cap, P->nzc);
  for (int i = 0; i < r; i++) ch->alphas[i] = dx_squeeze(&d);
  dx_absorb_cap(&d, (const F (*)[4])P->q_cap, P->nqc);
  ch->zeta = dx_squeeze_ext(&d);
  /* friChallenges, Challenge/FRI.hs:65-104 */
  int n1, n2; E* b1 = fri_batch_this(m, P, &n1); E* b2 = fri_batch_next(m, P, &n2);
  dx_absorb_exts(&d, b1, n1); dx_absorb_exts(&d, b2, n2);
  ch->fri_alpha = dx_squeeze_ext(&d);
  ch->nfri_betas = P->nccaps; ch->fri_betas = (E*)aalloc(m, (P->nccaps + 1) * sizeof(E));
  for (int i = 0; i < P->nccaps; i++) { dx_absorb_cap(&d, (const F (*)[4])P->ccaps[i], P->nccap[i]); ch->fri_betas[i] = dx_squeeze_ext(&d); }
  dx_absorb_exts(&d, P->final_poly, P->nfinal);
  dx_absorb(&d, P->pow_witness);
  ch->pow_response = dx_squeeze(&d);
  int lde_bits = C->degree_bits + C->rate_bits;
  ch->nquery = C->nqueries; ch->query_idx = (long*)aalloc(m, (C->nqueries + 1) * sizeof(long));
  for (int i = 0; i < C->nqueries; i++) { F f = dx_squeeze(&d); ch->query_idx[i] = (long)(lde_bits >= 64 ? f : (f & ((1ULL << lde_bits) - 1))); }
}

/* ================================================================ selectors
 * Gate/Selector.hs:31-95 */
typedef struct { int ngs, nls, ngc, nsig; } selcfg_t;
static selcfg_t get_selector_config(const circuit_t* C) {
  int expected = C->nluts == 0 ? 0 : 4 + C->nluts;
  if (C->nls != expected) fail(P2V_ERR_CIRCUIT, "getSelectorConfig: fatal: num_lookup_selectors /= (4 + #nluts)");
  if (C->num_constants != C->ngroups + C->nls + C->num_const_cfg) fail(P2V_ERR_CIRCUIT, "getSelectorConfig: fatal: constant columns tally does not add up!");
  selcfg_t s = { C->ngroups, C->nls, C->num_const_cfg, C->num_routed }; return s;
}
typedef struct { E* gsel; int ngsel; E* lsel; int nlsel; E* konst; int nkonst; } constcols_t;
static constcols_t split_constant_columns(selcfg_t s, E* xs, int n) {
  constcols_t c; int k = 0;
  c.gsel = xs; c.ngsel = s.ngs < n ? s.ngs : n; k = c.ngsel;
  c.lsel = xs + k; c.nlsel = s.nls < n - k ? s.nls : n - k; k += c.nlsel;
  c.konst = xs + k; c.nkonst = s.ngc < n - k ? s.ngc : n - k; k += c.nkonst;
  if (k != n) fail(P2V_ERR_SHAPE, "splitConstantColumns: fatal: numbers do not add up");
  if (c.nkonst != s.ngc) fail(P2V_ERR_SHAPE, "splitConstantColumns: fatal: not enough constant columns");
  return c;
}
static E eval_gate_selector_poly(const circuit_t* C, E x, int k) {
  if (k >= C->nsel_idx) fail(P2V_ERR_CIRCUIT, "selector_indices !! k");
  int g = C->sel_idx[k]; if (g < 0 || g >= C->ngroups) fail(P2V_ERR_CIRCUIT, "selector_groups !! group_idx");
  E unused = Eb(0xFFFFFFFFULL);
  E v = C->ngroups > 1 ? Esub(unused, x) : Eb(1);
  for (int j = C->grp_s[g]; j < C->grp_e[g]; j++) if (j != k) v = Emul(v, Esub(Eb((F)j % P_MOD), x));
  return v;
}

/* ============================================================ gate constraints
 * Gate/Constraints.hs:40-128 and Gate/Custom/ modules.  Each program is evaluated directly
 * over F^2 — the straight-line program of Gate/Computation.hs:117-164 only names
 * intermediate values, so direct evaluation gives the same field elements. */
typedef struct { const E* sel; int nsel; const E* lsel; int nlsel; const E* konst; int nkonst; const E* wires; int nwires; const F* pih; } evars_t;
typedef struct { E* v; int n, cap; arena* m; F* lutre; } clist;   /* lutre: evalFinalRE values for the trace */
static void cpush(clist* l, E x) {
  if (l->n == l->cap) { int nc = l->cap ? 2 * l->cap : 64; E* nv = (E*)aalloc(l->m, nc * sizeof(E)); if (l->n) memcpy(nv, l->v, l->n * sizeof(E)); l->v = nv; l->cap = nc; }
  l->v[l->n++] = x;
}
static void cpushx(clist* l, EE x) { cpush(l, x.re); cpush(l, x.im); }   /* commitExt Computation.hs:75-76 */
static E W(const evars_t* V, long long i) { if (i < 0 || i >= V->nwires) fail(P2V_ERR_CIRCUIT, "(Array.!): undefined array element (wire)"); return V->wires[i]; }
static E K(const evars_t* V, long long i) { if (i < 0 || i >= V->nkonst) fail(P2V_ERR_CIRCUIT, "(Array.!): undefined array element (constant)"); return V->konst[i]; }
static EE WX(const evars_t* V, long long i) { EE r = {W(V, i), W(V, i + 1)}; return r; }   /* wireExt Vars.hs:56-57 */
static E Lit(F x) { return Eb(x % P_MOD); }
static E Esbox(E x) { E x2 = Emul(x, x); E x3 = Emul(x, x2); E x4 = Emul(x2, x2); return Emul(x3, x4); }   /* Custom/Poseidon.hs:28-35 */

static void gate_poseidon(const evars_t* V, clist* out) {   /* Custom/Poseidon.hs:63-150 */
#define IN(i) W(V, (i))
#define OUT(i) W(V, (i) + 12)
#define SWAP W(V, 24)
#define DELTA(i) W(V, 25 + (i))
#define ISB(r, i) W(V, 29 + 12 * ((r) - 1) + (i))
#define PSB(r) W(V, 29 + 36 + (r))
#define FSB(r, i) W(V, 29 + 36 + 22 + 12 * (r) + (i))
  cpush(out, Emul(SWAP, Esub(SWAP, Eb(1))));
  for (int i = 0; i < 4; i++) cpush(out, Esub(Emul(SWAP, Esub(IN(i + 4), IN(i))), DELTA(i)));
  E st[12], t[12];
  for (int i = 0; i < 4; i++) st[i] = Eadd(IN(i), DELTA(i));
  for (int i = 4; i < 8; i++) st[i] = Esub(IN(i), DELTA(i - 4));
  for (int i = 8; i < 12; i++) st[i] = IN(i);
  for (int r = 0; r < 4; r++) {
    for (int i = 0; i < 12; i++) st[i] = Eadd(st[i], Lit(OR_ALL_ROUND_CONSTANTS[12 * r + i]));
    if (r != 0) { for (int i = 0; i < 12; i++) cpush(out, Esub(st[i], ISB(r, i))); for (int i = 0; i < 12; i++) st[i] = ISB(r, i); }
    for (int i = 0; i < 12; i++) st[i] = Esbox(st[i]);
    for (int i = 0; i < 12; i++) { E acc = Eb(0); for (int j = 0; j < 12; j++) acc = Eadd(acc, Emul(Lit(mds_coeff(i, j)), st[j])); t[i] = acc; }
    memcpy(st, t, sizeof st);
  }
  for (int i = 0; i < 12; i++) st[i] = Eadd(st[i], Lit(OR_FAST_PARTIAL_FIRST_ROUND_CONSTANT[i]));
  /* mdsInitPartial: partialMdsMatrixCoeff i j = INITIAL_MATRIX ! (j,i) (row-major) */
  t[0] = st[0];
  for (int i = 0; i < 11; i++) { E acc = Eb(0); for (int j = 0; j < 11; j++) acc = Eadd(acc, Emul(Lit(OR_FAST_PARTIAL_ROUND_INITIAL_MATRIX[11 * j + i]), st[1 + j])); t[1 + i] = acc; }
  memcpy(st, t, sizeof st);
  for (int r = 0; r < 22; r++) {
    cpush(out, Esub(st[0], PSB(r)));
    E y = Esbox(PSB(r));
    E z = r < 21 ? Eadd(y, Lit(OR_FAST_PARTIAL_ROUND_CONSTANTS[r])) : y;
    st[0] = z;
    /* mdsFastPartial r */
    E s0 = st[0];
    E dacc = Emul(st[0], Lit(mds_coeff(0, 0)));
    for (int j = 0; j < 11; j++) dacc = Eadd(dacc, Emul(st[1 + j], Lit(OR_FAST_PARTIAL_ROUND_W_HATS[11 * r + j])));
    t[0] = dacc;
    for (int j = 0; j < 11; j++) t[1 + j] = Eadd(st[1 + j], Emul(s0, Lit(OR_FAST_PARTIAL_ROUND_VS[11 * r + j])));
    memcpy(st, t, sizeof st);
  }
  for (int r = 0; r < 4; r++) {
    for (int i = 0; i < 12; i++) st[i] = Eadd(st[i], Lit(OR_ALL_ROUND_CONSTANTS[12 * (r + 26) + i]));
    for (int i = 0; i < 12; i++) cpush(out, Esub(st[i], FSB(r, i)));
    for (int i = 0; i < 12; i++) st[i] = Esbox(FSB(r, i));
    for (int i = 0; i < 12; i++) { E acc = Eb(0); for (int j = 0; j < 12; j++) acc = Eadd(acc, Emul(Lit(mds_coeff(i, j)), st[j])); t[i] = acc; }
    memcpy(st, t, sizeof st);
  }
  for (int i = 0; i < 12; i++) cpush(out, Esub(st[i], OUT(i)));
#undef IN
#undef OUT
#undef SWAP
#undef DELTA
#undef ISB
#undef PSB
#undef FSB
}

static void gate_coset(const evars_t* V, const gate_t* g, clist* out) {   /* Custom/CosetInterp.hs:51-121 */
  int bits = (int)g->p0; long long degree = g->p1;
  long long npts = 1LL << bits;
  if (degree - 1 == 0) fail(P2V_ERR_CIRCUIT, "divide by zero (CosetInterpolationGate degree)");
  long long nint = (npts - 2) / (degree - 1);
  /* Haskell `div` floors */
  if ((npts - 2) % (degree - 1) != 0 && ((npts - 2) < 0) != ((degree - 1) < 0)) nint -= 1;
  F gen = subgroup_gen(bits);
  E shift = W(V, 0);
#define VAL(k) WX(V, 1 + 2 * (k))
  EE eval_loc = WX(V, 1 + 2 * npts), eval_result = WX(V, 1 + 2 * npts + 2);
  EE shifted = WX(V, 1 + 2 * (npts + 2) + 4 * nint);
  cpushx(out, EEsub(eval_loc, EEscale(shift, shifted)));
  /* chunk xs = take degree xs : partition (degree-1) (drop degree xs) */
  long long nchunks = 0; long long cs[4096], ce[4096];
  {
    long long first = degree < npts ? degree : npts; if (first < 0) first = 0;
    cs[0] = 0; ce[0] = first; nchunks = 1;
    long long pos = first;
    while (pos < npts) { long long e = pos + (degree - 1); if (e > npts) e = npts; cs[nchunks] = pos; ce[nchunks] = e; nchunks++; pos = e; if (degree - 1 <= 0) fail(P2V_ERR_CIRCUIT, "partition: non-positive chunk"); }
  }
  /* chunks = zip3 chunked_domain chunked_values chunked_weights: a short weight list has fewer chunks */
  {
    long long nw = g->nweights, wfirst = degree < nw ? degree : nw;
    long long nchunks_w = 1 + (nw - wfirst + (degree - 2)) / (degree - 1);
    if (nchunks_w < nchunks) nchunks = nchunks_w;
  }
  long long nst = nint + 1 < nchunks ? nint + 1 : nchunks;   /* zipWith worker initials chunks */
  EE* evs = (EE*)malloc((nst + 1) * sizeof(EE)); EE* prs = (EE*)malloc((nst + 1) * sizeof(EE));
  for (long long c = 0; c < nst; c++) {
    EE ev, pr;
    if (c == 0) { ev.re = Eb(0); ev.im = Eb(0); pr.re = Eb(1); pr.im = Eb(0); }
    else { ev = WX(V, 1 + 2 * (npts + 2) + 2 * (c - 1)); pr = WX(V, 1 + 2 * (npts + 2) + 2 * (nint + c - 1)); }
    F x = 1; for (long long k = 0; k < cs[c]; k++) x = fmul(x, gen);
    for (long long k = cs[c]; k < ce[c]; k++) {
      if (k >= g->nweights) break;   /* zipWith scaleExt weights values truncates */
      EE val = EEscale(Eb(g->weights[k]), VAL(k));
      EE term = EEsub(shifted, EEfromBase(Eb(x)));
      EE ne = EEadd(EEmul(term, ev), EEmul(val, pr));
      pr = EEmul(term, pr); ev = ne;
      x = fmul(x, gen);
    }
    evs[c] = ev; prs[c] = pr;
  }
  for (long long i = 0; i + 1 < nst; i++) {
    cpushx(out, EEsub(WX(V, 1 + 2 * (npts + 2) + 2 * i), evs[i]));
    cpushx(out, EEsub(WX(V, 1 + 2 * (npts + 2) + 2 * (nint + i)), prs[i]));
  }
  if (nst == 0) fail(P2V_ERR_CIRCUIT, "Prelude.last: empty list");
  cpushx(out, EEsub(eval_result, evs[nst - 1]));
  free(evs); free(prs);
#undef VAL
}

static void gate_random_access(const evars_t* V, const gate_t* g, clist* out) {   /* Custom/RandomAccess.hs:47-88 */
  int nbits = (int)g->p0; long long copies = g->p1, extra = g->p2;
  long long veclen = 1LL << nbits, width = 2 + veclen;
  long long bstart = width * copies + extra;
  for (long long k = 0; k < copies; k++) {
    for (int j = 0; j < nbits; j++) { E b = W(V, bstart + k * nbits + j); cpush(out, Emul(b, Esub(b, Eb(1)))); }
    E rec = Eb(0);
    for (int j = nbits - 1; j >= 0; j--) rec = Eadd(Emul(Eb(2), rec), W(V, bstart + k * nbits + j));   /* foldr (\b acc -> 2*acc + b) 0 */
    cpush(out, Esub(rec, W(V, k * width + 0)));
    E* vals = (E*)malloc(veclen * sizeof(E)); int nv = (int)veclen;
    for (long long i = 0; i < veclen; i++) vals[i] = W(V, k * width + 2 + i);
    for (int j = 0; j < nbits; j++) {
      E b = W(V, bstart + k * nbits + j);
      if (nv & 1) fail(P2V_ERR_CIRCUIT, "into_pairs: odd input");
      for (int t = 0; t < nv / 2; t++) { E x = vals[2 * t], y = vals[2 * t + 1]; vals[t] = Eadd(x, Emul(b, Esub(y, x))); }
      nv /= 2;
    }
    if (nv != 1) fail(P2V_ERR_CIRCUIT, "RandomAccessGate/lookup_eq: shouldn't happen");
    cpush(out, Esub(vals[0], W(V, k * width + 1)));
    free(vals);
  }
  for (long long j = 0; j < extra; j++) cpush(out, Esub(K(V, j), W(V, copies * width + j)));
}

static void gate_constraints(const gate_t* g, const evars_t* V, clist* out) {
  switch (g->kind) {
    case G_ARITH:   /* Constraints.hs:45-46 */
      for (long long i = 0; i < g->p0; i++) { long long j = 4 * i;
        cpush(out, Esub(Esub(W(V, j + 3), Emul(Emul(K(V, 0), W(V, j)), W(V, j + 1))), Emul(K(V, 1), W(V, j + 2)))); }
      break;
    case G_ARITH_EXT:   /* :49-54 */
      for (long long i = 0; i < g->p0; i++) { long long j = 8 * i;
        EE c0 = EEfromBase(K(V, 0)), c1 = EEfromBase(K(V, 1));
        cpushx(out, EEsub(EEsub(WX(V, j + 6), EEmul(EEmul(c0, WX(V, j)), WX(V, j + 2))), EEmul(c1, WX(V, j + 4)))); }
      break;
    case G_BASESUM: {   /* :57-62 */
      long long nl = g->p0; E base = Lit((F)g->p1);
      long long k = nl - 1 > 0 ? nl - 1 : 0;
      /* go k = if k < nl-1 then limb k + base * go (k+1) else limb k */
      E h;
      if (0 < nl - 1) { h = W(V, (nl - 1) + 1); for (long long t = nl - 2; t >= 0; t--) h = Eadd(W(V, t + 1), Emul(base, h)); }
      else h = W(V, 0 + 1);
      (void)k;
      cpush(out, Esub(h, W(V, 0)));
      for (long long i = 0; i < nl; i++) { E pr = Eb(1); for (long long t = 0; t < g->p1; t++) pr = Emul(pr, Esub(W(V, i + 1), Lit((F)t))); cpush(out, pr); }
      break; }
    case G_COSET: gate_coset(V, g, out); break;
    case G_CONST: for (long long i = 0; i < g->p0; i++) cpush(out, Esub(K(V, i), W(V, i))); break;   /* :68-69 */
    case G_EXP: {   /* :114-128 */
      long long n = g->p0;
      for (long long i = 0; i < n; i++) {
        E prev = i == 0 ? Eb(1) : Emul(W(V, n + 2 + i - 1), W(V, n + 2 + i - 1));
        E bit = W(V, (n - 1 - i) + 1);
        E comp = Emul(prev, Eadd(Emul(bit, W(V, 0)), Esub(Eb(1), bit)));
        cpush(out, Esub(comp, W(V, n + 2 + i)));
      }
      cpush(out, Esub(W(V, n + 1), W(V, n + 2 + n - 1)));
      break; }
    case G_LOOKUP: case G_LOOKUPTABLE: case G_NOOP: break;
    case G_MULEXT:   /* :80-83 */
      for (long long i = 0; i < g->p0; i++) { long long j = 6 * i;
        cpushx(out, EEsub(WX(V, j + 4), EEmul(EEmul(EEfromBase(K(V, 0)), WX(V, j)), WX(V, j + 2)))); }
      break;
    case G_PI: for (int i = 0; i < 4; i++) cpush(out, Esub(W(V, i), Eb(V->pih[i]))); break;   /* :88-89 */
    case G_POSEIDON: if (g->p0 != 12) fail(P2V_ERR_CIRCUIT, "gateConstraints/PoseidonGate: unsupported width"); gate_poseidon(V, out); break;
    case G_POSEIDON_MDS:   /* Custom/Poseidon.hs:49-59 */
      if (g->p0 != 12) fail(P2V_ERR_CIRCUIT, "gateConstraints/PoseidonMdsGate: unsupported width");
      for (int i = 0; i < 12; i++) {
        EE acc = {Eb(0), Eb(0)};
        for (int j = 0; j < 12; j++) acc = EEadd(acc, EEscale(Lit(mds_coeff(i, j)), WX(V, 2 * j)));
        cpushx(out, EEsub(WX(V, 2 * (i + 12)), acc));
      }
      break;
    case G_RANDACC: gate_random_access(V, g, out); break;
    case G_REDUCING: {   /* Custom/Reducing.hs:28-41 */
      long long n = g->p0;
      for (long long i = 0; i < n; i++) {
        EE prev = i == 0 ? WX(V, 4) : (i - 1 < n - 1 ? WX(V, 6 + n + 2 * (i - 1)) : WX(V, 0));
        EE acc = i < n - 1 ? WX(V, 6 + n + 2 * i) : WX(V, 0);
        cpushx(out, EEsub(EEadd(EEmul(prev, WX(V, 2)), EEfromBase(W(V, 6 + i))), acc));
      }
      break; }
    case G_REDUCING_EXT: {   /* Custom/Reducing.hs:45-60 */
      long long n = g->p0;
      for (long long i = 0; i < n; i++) {
        EE prev = i == 0 ? WX(V, 4) : (i - 1 < n - 1 ? WX(V, 6 + 2 * n + 2 * (i - 1)) : WX(V, 0));
        EE acc = i < n - 1 ? WX(V, 6 + 2 * n + 2 * i) : WX(V, 0);
        cpushx(out, EEsub(EEadd(EEmul(prev, WX(V, 2)), WX(V, 6 + 2 * i)), acc));
      }
      break; }
    default: fail(P2V_ERR_CIRCUIT, "gateConstraints: unknown gate");
  }
}

/* =============================================================== lookups
 * Plonk/Lookups.hs:45-132 */
static void eval_lookup_equations(const circuit_t* C, const constcols_t* cc, const proof_t* P, const chal_t* ch, clist* out) {
  int nlp = C->nlp;
#define SEL(idx) ((idx) < cc->nlsel ? (ch->unit_filters ? Eb(1) : cc->lsel[(idx)]) : (fail(P2V_ERR_SHAPE, "Prelude.!!: index too large (lookup selector)"), E0()))
  int npairs = P->n_lzs < P->n_lzs_next ? P->n_lzs : P->n_lzs_next;   /* zip */
  if (nlp <= 0) fail(P2V_ERR_CIRCUIT, "partition: non-positive lookup chunk");
  int nchunks = (npairs + nlp - 1) / nlp;
  if (nchunks != ch->ndeltas) fail(P2V_ERR_SHAPE, "safeZipWith: different input lengths");
  int num_lu_slots = C->num_routed / 2, num_lut_slots = C->num_routed / 3;
  int nsldc = nlp - 1, lu_degree = C->qdf - 1;
  if (nsldc <= 0) fail(P2V_ERR_CIRCUIT, "divide by zero (num_sldc_polys)");
  int lut_degree = (num_lut_slots + nsldc - 1) / nsldc;
  for (int rr = 0; rr < nchunks; rr++) {
    const ldelta_t* D = &ch->deltas[rr];
    int s = rr * nlp, e = s + nlp < npairs ? s + nlp : npairs;
    if (e <= s) fail(P2V_ERR_SHAPE, "irrefutable pattern (re_pair:sldc_pairs)");
    E re = P->o_lzs[s], re_next = P->o_lzs_next[s];
    int ns = e - s - 1; const E* sldc = P->o_lzs + s + 1; const E* sldc_next = P->o_lzs_next + s + 1;
    /* lu_combos / lut_combos over partition 2 / 3 of the wires (list-comprehension pattern skips short chunks) */
    int nlu = 0, nlut = 0;
    E lu[512], lutA[512], lutB[512], mults[512];
    for (int t = 0; t < num_lu_slots && 2 * t + 1 < P->n_wires; t++) { lu[nlu++] = Eadd(P->o_wires[2 * t], Escale(D->A, P->o_wires[2 * t + 1])); }
    for (int t = 0; t < num_lut_slots && 3 * t + 2 < P->n_wires; t++) {
      lutA[nlut] = Eadd(P->o_wires[3 * t], Escale(D->A, P->o_wires[3 * t + 1]));
      lutB[nlut] = Eadd(P->o_wires[3 * t], Escale(D->B, P->o_wires[3 * t + 1])); nlut++;
    }
    for (int t = 0; t < num_lut_slots; t++) { if (3 * t + 2 >= P->n_wires) fail(P2V_ERR_SHAPE, "Prelude.!!: index too large (mult)"); mults[t] = P->o_wires[3 * t + 2]; }
    if (ns <= 0) fail(P2V_ERR_SHAPE, "Prelude.last: empty list");
    cpush(out, Emul(SEL(3), sldc[ns - 1]));       /* eq_last_sldc */
    cpush(out, Emul(SEL(2), sldc[0]));            /* eq_ini_sum  */
    cpush(out, Emul(SEL(2), re));                 /* eq_ini_re   */
    for (int k = 0; k < C->nluts; k++) {          /* eq_finals_re, evalFinalRE :103-109 */
      int len = C->lut_len[k];
      if (num_lut_slots == 0) fail(P2V_ERR_CIRCUIT, "divide by zero (num_lut_slots)");
      int nrows = (len + num_lut_slots - 1) / num_lut_slots; long padded = (long)nrows * num_lut_slots;
      F cur = 0;
      for (long i = 0; i < padded; i++) {
        long j = i < len ? i : 0;   /* lut ++ repeat (head lut) */
        F x = fadd(C->lut_in[k][j], fmul(D->B, C->lut_out[k][j]));
        cur = fadd(fmul(D->delta, cur), x);
      }
      if (out->lutre) out->lutre[rr * C->nluts + k] = cur;
      cpush(out, Emul(SEL(4 + k), Esub(re, Eb(cur))));
    }
    {   /* eq_re_trans */
      E cs = re_next;
      for (int t = 0; t < nlut; t++) cs = Eadd(Escale(D->delta, cs), lutB[t]);
      cpush(out, Emul(SEL(0), Esub(re, cs)));
    }
    /* eqs_sldc: zip (pairs (last sldc_next : sldc)) (zip3 chunks_lu chunks_lut chunks_mults) */
    int nprev = ns;   /* pairs of a list of length ns+1 */
    int nclu = (nlu + lu_degree - 1) / lu_degree, nclut = (nlut + lut_degree - 1) / lut_degree, ncm = (num_lut_slots + lut_degree - 1) / lut_degree;
    if (lu_degree <= 0) fail(P2V_ERR_CIRCUIT, "partition: non-positive lu_degree");
    int nz = nclu < nclut ? nclu : nclut; nz = nz < ncm ? nz : ncm; nz = nz < nprev ? nz : nprev;
    E alpha = Eb(D->alpha);
    for (int c = 0; c < nz; c++) {
      E prev = c == 0 ? sldc_next[ns - 1] : sldc[c - 1];
      E cur = sldc[c];
      int ls = c * lu_degree, le = ls + lu_degree < nlu ? ls + lu_degree : nlu;
      int ts = c * lut_degree, te = ts + lut_degree < nlut ? ts + lut_degree : nlut;
      int ms = c * lut_degree, me = ms + lut_degree < num_lut_slots ? ms + lut_degree : num_lut_slots;
      E lu_prod = Eb(1), lut_prod = Eb(1);
      for (int t = ls; t < le; t++) lu_prod = Emul(lu_prod, Esub(alpha, lu[t]));
      for (int t = ts; t < te; t++) lut_prod = Emul(lut_prod, Esub(alpha, lutA[t]));
      if (le <= ls || te <= ts) fail(P2V_ERR_CIRCUIT, "select1: empty list");
      E lu_sum = Eb(0), lut_sum = Eb(0);
      for (int o = ls; o < le; o++) { E pr = Eb(1); for (int t = ls; t < le; t++) if (t != o) pr = Emul(pr, Esub(alpha, lu[t])); lu_sum = Eadd(lu_sum, pr); }
      int nmz = (te - ts) < (me - ms) ? (te - ts) : (me - ms);   /* zip mults (remove1 lut_combos) */
      for (int o = 0; o < nmz; o++) { E pr = mults[ms + o]; for (int t = ts; t < te; t++) if (t != ts + o) pr = Emul(pr, Esub(alpha, lutA[t])); lut_sum = Eadd(lut_sum, pr); }
      E diff = Esub(cur, prev);
      cpush(out, Emul(SEL(0), Esub(Emul(lut_prod, diff), lut_sum)));   /* eq_sum_trans */
      cpush(out, Emul(SEL(1), Eadd(Emul(lu_prod, diff), lu_sum)));     /* eq_ldc_trans */
    }
  }
#undef SEL
}

/* ================================================================ vanishing
 * Plonk/Vanishing.hs:48-137, Algebra/Poly.hs:14-16 */
static E eval_lagrange0(long nn, E zeta) {
  if (Eeq(zeta, Eb(1))) return Eb(1);
  return Ediv(Esub(Epow(zeta, nn), Eb(1)), Emul(Eb((F)nn % P_MOD), Esub(zeta, Eb(1))));
}

static void eval_all_constraints(arena* m, const circuit_t* C, const proof_t* P, const chal_t* ch, clist* out) {
  selcfg_t sc = get_selector_config(C);
  constcols_t cc = split_constant_columns(sc, P->o_const, P->n_const);
  long nn = 1L << C->degree_bits; int maxdeg = C->qdf;
  /* zs1 */
  E L0 = eval_lagrange0(nn, ch->zeta);
  for (int i = 0; i < P->n_zs; i++) cpush(out, Emul(L0, Esub(P->o_zs[i], Eb(1))));
  /* pp_checks: zipWith4 evalPartialProducts zs zs_next (zip betas gammas) pp_chunks */
  if (C->npp <= 0 && P->n_pp > 0) fail(P2V_ERR_CIRCUIT, "partition: non-positive num_partial_products");
  int npc = C->npp > 0 ? (P->n_pp + C->npp - 1) / C->npp : 0;
  int nz = P->n_zs; if (P->n_zs_next < nz) nz = P->n_zs_next; if (C->r < nz) nz = C->r; if (npc < nz) nz = npc;
  if (maxdeg <= 0) fail(P2V_ERR_CIRCUIT, "partition: non-positive quotient_degree_factor");
  for (int i = 0; i < nz; i++) {
    F beta = ch->betas[i], gamma = ch->gammas[i];
    int nnum = C->nk < P->n_wires ? C->nk : P->n_wires;
    int nden = P->n_sig < P->n_wires ? P->n_sig : P->n_wires;
    int cs = i * C->npp, ce = cs + C->npp < P->n_pp ? cs + C->npp : P->n_pp;
    int ncur = 1 + (ce - cs) + 1;   /* [z] ++ pp_chunk ++ [znext] */
    E* cur = (E*)malloc(ncur * sizeof(E));
    cur[0] = P->o_zs[i]; for (int t = cs; t < ce; t++) cur[1 + t - cs] = P->o_pp[t]; cur[ncur - 1] = P->o_zs_next[i];
    int nnc = (nnum + maxdeg - 1) / maxdeg, ndc = (nden + maxdeg - 1) / maxdeg;
    int nt = ncur - 1; if (nnc < nt) nt = nnc; if (ndc < nt) nt = ndc;
    for (int c = 0; c < nt; c++) {
      E pn = Eb(1), pd = Eb(1);
      for (int t = c * maxdeg; t < nnum && t < (c + 1) * maxdeg; t++)
        pn = Emul(pn, Eadd(Eadd(P->o_wires[t], Escale(fmul(beta, C->k_is[t]), ch->zeta)), Eb(gamma)));
      for (int t = c * maxdeg; t < nden && t < (c + 1) * maxdeg; t++)
        pd = Emul(pd, Eadd(Eadd(P->o_wires[t], Escale(beta, P->o_sig[t])), Eb(gamma)));
      cpush(out, Esub(Emul(cur[c], pn), Emul(cur[c + 1], pd)));
    }
    free(cur);
  }
  /* lookups */
  if (C->nluts > 0) eval_lookup_equations(C, &cc, P, ch, out);
  /* gates: filtered = zipWith (\s cons -> map (*s) cons) sel_values unfiltered; vertical sum */
  evars_t V = { cc.gsel, cc.ngsel, cc.lsel, cc.nlsel, cc.konst, cc.nkonst, P->o_wires, P->n_wires, ch->pi_hash };
  int ng = C->nsel_idx < C->ngates ? C->nsel_idx : C->ngates;
  if (ng == 0) fail(P2V_ERR_CIRCUIT, "foldl1: empty list (no gates)");
  clist sum = {0}; sum.m = m;
  for (int g = 0; g < ng; g++) {
    int grp = C->sel_idx[g];
    if (grp < 0 || grp >= cc.ngsel) fail(P2V_ERR_CIRCUIT, "Prelude.!!: index too large (selector column)");
    E s = ch->unit_filters ? Eb(1) : eval_gate_selector_poly(C, cc.gsel[grp], g);
    clist cons = {0}; cons.m = m;
    gate_constraints(&C->gates[g], &V, &cons);
    for (int k = 0; k < cons.n; k++) {
      E f = Emul(cons.v[k], s);
      if (k < sum.n) sum.v[k] = Eadd(sum.v[k], f); else cpush(&sum, f);   /* longZipWith 0 0 (+) */
    }
  }
  for (int k = 0; k < sum.n; k++) cpush(out, sum.v[k]);
}

/* ===================================================================== FRI
 * Plonk/FRI.hs:56-407 */
/* SALT_SIZE trailing salts of the wires / zs / quotient leaves under P2V_EXT_HIDING (plonky2
 * FriInitialTreeProof::unsalted_evals); the reference has none (Plonk/FRI.hs:56-75) */
static int leaf_salt(const circuit_t* C, int t) { return (C->ext & 2u) && C->hiding && t > 0 ? 4 : 0; }
static int oracle_width(const circuit_t* C, int t) {   /* oracleWidths :56-65 */
  switch (t) {
    case 0: return C->num_constants + C->num_routed;
    case 1: return C->num_wires;
    case 2: return C->r * (1 + C->npp + C->nlp);
    default: return C->r * C->qdf;
  }
}
static int expand_strategy(const circuit_t* C, int* arities) {   /* expandReductionStrategy :337-354 */
  int n = 0;
  if (C->ext & 1u) {   /* P2V_EXT_PARAMS_ARITIES: plonky2 reads fri_params.reduction_arity_bits */
    for (int i = 0; i < C->nparams_ar && i < 64; i++) arities[n++] = C->params_ar[i];
    return n;
  }
  if (C->strat == 0) { int logn = C->degree_bits; while (logn > C->strat_b) { if (n >= 64) fail(P2V_ERR_CIRCUIT, "reduction strategy does not terminate"); arities[n++] = C->strat_a; logn -= C->strat_a; } }
  else if (C->strat == 1) { for (int i = 0; i < C->nfixed && i < 64; i++) arities[n++] = C->fixed[i]; }
  else fail(P2V_ERR_CIRCUIT, "reduction strategy not implemented");
  return n;
}

/* foldCosetWith, :263-279: interpolant through the coset points evaluated at beta,
 * computed exactly as written (sum over k of beta^k (1/arity) sum_j x_j^-k v_j). */
static E fold_coset(E beta, int arity_bits, F ofs, const E* vals_bitrev) {
  int arity = 1 << arity_bits;
  F omega = subgroup_gen(arity_bits);
  F inv_arity = fdiv(1, (F)arity);
  E acc = Eb(0), bk = Eb(1);
  for (int k = 0; k < arity; k++) {
    E y = Eb(0);
    for (int j = 0; j < arity; j++) {
      F xj = fmul(ofs, fpow(omega, (u128)j));
      y = Eadd(y, Escale(fpow_i(xj, -(long long)k), vals_bitrev[j]));
    }
    acc = Eadd(acc, Emul(bk, y)); bk = Emul(bk, beta);
  }
  return Escale(inv_arity, acc);
}

typedef struct { E initial, folded, final; int code; } qres_t;
static void trace_put(uint64_t* tr, long off, F v) { if (tr) tr[off] = v; }

/* checkQueryRound, :381-407 — returns the per-round outcome code; fills values even
 * past a failing check (the trace is for parity debugging only). */
static void check_query_round(const circuit_t* C, const proof_t* P, const chal_t* ch, E y0, E y1,
                              const int* arities, int nsteps, int qi, qres_t* res, int strict) {
  long idx = ch->query_idx[qi];
  const qround_t* R = &P->rounds[qi];
  int lde_bits = C->degree_bits + C->rate_bits;
  res->code = 1;
  /* checkInitialTreeProofs :105-117 */
  if (R->ninit != 4) fail(P2V_ERR_SHAPE, "checkInitialTreeProofs: expecting 4 Merkle proofs for the 4 oracles");
  const F (*caps[4])[4] = { (const F (*)[4])C->cs_cap, (const F (*)[4])P->wires_cap, (const F (*)[4])P->zs_cap, (const F (*)[4])P->q_cap };
  int ncaps[4] = { C->ncs_cap, P->nwc, P->nzc, P->nqc };
  for (int t = 0; t < 4; t++) if (ncaps[t] != (1 << C->cap_height)) fail(P2V_ERR_SHAPE, "validateMerkleCapLength: cap has wrong size");
  int merkle_ok = 1;   /* and [...] short-circuits */
  const int noop = (C->ext & 4u) != 0;
  for (int t = 0; t < 4 && (merkle_ok || !strict); t++) if (!check_merkle(caps[t], ncaps[t], idx, R->init[t].leaf, R->init[t].nleaf, (const F (*)[4])R->init[t].sib, R->init[t].nsib, noop)) merkle_ok = 0;
  if (!merkle_ok) { res->code = P2V_ERR_INITIAL_MERKLE; if (strict) return; }
  for (int t = 0; t < 4; t++) if (R->init[t].nleaf != oracle_width(C, t) + leaf_salt(C, t)) fail(P2V_ERR_SHAPE, "buildListOracle: list size do not match the expected");
  /* combineInitial :151-207 */
  int r = C->r;
  int npp = (C->num_routed + C->qdf - 1) / C->qdf;
  if (r * (npp + C->nlp) != oracle_width(C, 2)) fail(P2V_ERR_CIRCUIT, "combineInitial: sanity check failed");
  const F* oc = R->init[0].leaf; const F* ow = R->init[1].leaf; const F* opl = R->init[2].leaf; const F* oq = R->init[3].leaf;
  int noc = R->init[0].nleaf - leaf_salt(C, 0), now = R->init[1].nleaf - leaf_salt(C, 1),
      npl = R->init[2].nleaf - leaf_salt(C, 2), noq = R->init[3].nleaf - leaf_salt(C, 3);   /* unsalted */
  int nppo = r * npp < npl ? r * npp : npl;
  int len1 = noc + now + nppo + noq + (npl - nppo);
  int len2 = (r < nppo ? r : nppo) + (npl - nppo);
  F* b1 = (F*)malloc((len1 + 1) * 8); F* b2 = (F*)malloc((len2 + 1) * 8); int k = 0;
  memcpy(b1 + k, oc, noc * 8); k += noc; memcpy(b1 + k, ow, now * 8); k += now; memcpy(b1 + k, opl, nppo * 8); k += nppo;
  memcpy(b1 + k, oq, noq * 8); k += noq; memcpy(b1 + k, opl + nppo, (npl - nppo) * 8);
  k = 0; memcpy(b2, opl, (r < nppo ? r : nppo) * 8); k = r < nppo ? r : nppo; memcpy(b2 + k, opl + nppo, (npl - nppo) * 8);
  E g0 = Eb(0), g1 = Eb(0);
  for (int i = len1 - 1; i >= 0; i--) g0 = Eadd(Eb(b1[i]), Emul(ch->fri_alpha, g0));   /* reduceWithPowers :180-183 */
  for (int i = len2 - 1; i >= 0; i--) g1 = Eadd(Eb(b2[i]), Emul(ch->fri_alpha, g1));
  free(b1); free(b2);
  F omega = subgroup_gen(C->degree_bits), eta = subgroup_gen(lde_bits);
  F px = fmul(MULT_GEN, fpow(eta, rev_bits(lde_bits, (uint64_t)idx)));
  E one = Ediv(Esub(g0, y0), Esub(Eb(px), ch->zeta));
  E two = Ediv(Esub(g1, y1), Esub(Eb(px), Escale(omega, ch->zeta)));
  E cur = Eadd(Emul(Epow(ch->fri_alpha, len2), one), two);
  res->initial = cur;
  /* folding, :233-323 */
  if (nsteps != ch->nfri_betas || nsteps != P->nccaps || nsteps != R->nsteps) fail(P2V_ERR_SHAPE, "safeZipWith4: different input lengths");
  F shift = MULT_GEN; int logn = lde_bits; long qidx = idx;
  for (int s = 0; s < nsteps; s++) {
    const step_t* S = &R->steps[s];
    int ab = arities[s], arity = 1 << ab;
    long nidx = qidx >> ab;
    F* flat = (F*)malloc((2 * S->nevals + 1) * 8);
    for (int i = 0; i < S->nevals; i++) { flat[2 * i] = S->evals[i].a; flat[2 * i + 1] = S->evals[i].b; }
    int ok_m = check_merkle((const F (*)[4])P->ccaps[s], P->nccap[s], nidx, flat, 2 * S->nevals, (const F (*)[4])S->sib, S->nsib, noop);
    free(flat);
    if (res->code == 1 && !ok_m) { res->code = P2V_ERR_STEP_MERKLE; if (strict) return; }
    long pos = qidx % arity;
    if (pos >= S->nevals) fail(P2V_ERR_SHAPE, "Prelude.!!: index too large (evals)");
    int ok_e = Eeq(S->evals[pos], cur);
    if (res->code == 1 && !ok_e) { res->code = P2V_ERR_STEP_EVAL; if (strict) return; }
    int sz = S->nevals, lg = -1; for (int b = 0; b < 31; b++) if ((1 << b) == sz) lg = b;
    if (lg < 0) fail(P2V_ERR_SHAPE, "safeLog2: input is not a power of two");
    if (res->code == 1 && lg != ab) { res->code = P2V_ERR_STEP_ARITY; if (strict) return; }
    /* prepareCoset :248-259 (uses the length of `values`, not the strategy arity) */
    F eta_b = subgroup_gen(logn);
    long start = (long)rev_bits(logn, (uint64_t)((qidx >> lg) << lg));
    F ofs = fmul(shift, fpow(eta_b, (u128)start));
    E* vb = (E*)malloc(sz * sizeof(E));
    for (int i = 0; i < sz; i++) vb[rev_bits(lg, (uint64_t)i)] = S->evals[i];
    cur = fold_coset(ch->fri_betas[s], lg, ofs, vb);
    free(vb);
    shift = fpow(shift, (u128)arity);
    qidx = nidx; logn -= ab;
  }
  res->folded = cur;
  /* final polynomial, :288-291,325-327,404-407 */
  F eta_f = subgroup_gen(logn);
  F xf = fmul(shift, fpow(eta_f, rev_bits(logn, (uint64_t)qidx)));
  E acc = Eb(0), pw = Eb(1);
  for (int i = 0; i < P->nfinal; i++) { acc = Eadd(acc, Emul(P->final_poly[i], pw)); pw = Emul(pw, Eb(xf)); }
  res->final = acc;
  if (res->code == 1 && !Eeq(acc, cur)) res->code = P2V_REJECT;
}

/* ========================================================================= verify
 * verifyProof, Plonk/Verifier.hs:56-65:  eqs_ok && fri_ok */
typedef struct or_circuit { circuit_t c; } or_circuit;
typedef struct or_proof { proof_t p; } or_proof;


/* trace values for one query: lenient recomputation (checks do not stop it), shape
 * errors swallowed; runs in its own frame so its longjmp cannot clobber the caller. */
__attribute__((noinline)) static void trace_query(const circuit_t* C, const proof_t* P, const chal_t* ch, E y0, E y1, const int* arities,
                        int nsteps, int q, uint64_t* tr, long o_qin, long o_qf, long o_qfin) {
  qres_t res; memset(&res, 0, sizeof res);
  jmp_buf jq; jmp_buf* volatile sv = g_jb; int scode = g_code; char smsg[512]; memcpy(smsg, g_msg, sizeof smsg);
  g_jb = &jq;
  if (setjmp(jq)) { g_jb = sv; g_code = scode; memcpy(g_msg, smsg, sizeof smsg); return; }
  check_query_round(C, P, ch, y0, y1, arities, nsteps, q, &res, 0);
  g_jb = sv; g_code = scode; memcpy(g_msg, smsg, sizeof smsg);
  trace_put(tr, o_qin + 2 * q, res.initial.a); trace_put(tr, o_qin + 2 * q + 1, res.initial.b);
  trace_put(tr, o_qf + 2 * q, res.folded.a); trace_put(tr, o_qf + 2 * q + 1, res.folded.b);
  trace_put(tr, o_qfin + 2 * q, res.final.a); trace_put(tr, o_qfin + 2 * q + 1, res.final.b);
}

static int verify_body(const circuit_t* C, const proof_t* P, uint64_t* tr, int full_trace, arena* mp);
static int verify_impl(const circuit_t* C, const proof_t* P, uint64_t* tr, int full_trace) {
  arena m = {0};
  jmp_buf jb; jmp_buf* saved = g_jb; g_jb = &jb;
  if (setjmp(jb)) { afree(&m); g_jb = saved; return g_code; }
  int status = verify_body(C, P, tr, full_trace, &m);
  afree(&m); g_jb = saved;
  return status;
}
__attribute__((noinline)) static int verify_body(const circuit_t* C, const proof_t* P, uint64_t* tr, int full_trace, arena* mp) {
  arena* m_ = mp; (void)full_trace;
  int status;
  chal_t ch; memset(&ch, 0, sizeof ch);
  proof_challenges(m_, C, P, &ch);
  ch.unit_filters = (full_trace & 2) != 0;
  int r = C->r, Q = C->nqueries;
  int arities[64]; int nsteps = expand_strategy(C, arities);
  long o_pi = 0, o_b = 4, o_g = o_b + r, o_a = o_g + r, o_d = o_a + r, o_z = o_d + 4 * r, o_fa = o_z + 2, o_fb = o_fa + 2,
       o_pw = o_fb + 2 * nsteps, o_qi = o_pw + 1, o_c = o_qi + Q, o_q = o_c + 2 * r, o_qin = o_q + 2 * r, o_qf = o_qin + 2 * Q,
       o_qfin = o_qf + 2 * Q, o_fl = o_qfin + 2 * Q;
  if (tr) {
    memset(tr, 0, (size_t)P2V_TRACE_WORDS(r, nsteps, Q, C->nluts) * 8);
    for (int i = 0; i < 4; i++) trace_put(tr, o_pi + i, ch.pi_hash[i]);
    for (int i = 0; i < r; i++) { trace_put(tr, o_b + i, ch.betas[i]); trace_put(tr, o_g + i, ch.gammas[i]); trace_put(tr, o_a + i, ch.alphas[i]); }
    for (int i = 0; i < ch.ndeltas && i < r; i++) { trace_put(tr, o_d + 4 * i, ch.deltas[i].A); trace_put(tr, o_d + 4 * i + 1, ch.deltas[i].B); trace_put(tr, o_d + 4 * i + 2, ch.deltas[i].alpha); trace_put(tr, o_d + 4 * i + 3, ch.deltas[i].delta); }
    trace_put(tr, o_z, ch.zeta.a); trace_put(tr, o_z + 1, ch.zeta.b); trace_put(tr, o_fa, ch.fri_alpha.a); trace_put(tr, o_fa + 1, ch.fri_alpha.b);
    for (int i = 0; i < ch.nfri_betas && i < nsteps; i++) { trace_put(tr, o_fb + 2 * i, ch.fri_betas[i].a); trace_put(tr, o_fb + 2 * i + 1, ch.fri_betas[i].b); }
    trace_put(tr, o_pw, ch.pow_response);
    for (int i = 0; i < Q; i++) trace_put(tr, o_qi + i, (F)ch.query_idx[i]);
  }
  /* eqs_ok: checkCombinedPlonkEquations', Plonk/Verifier.hs:35-51 */
  clist cons = {0}; cons.m = m_;
  if (tr && C->nluts > 0) cons.lutre = (F*)aalloc(m_, (size_t)r * C->nluts * sizeof(F));
  if (cons.lutre) memset(cons.lutre, 0, (size_t)r * C->nluts * sizeof(F));
  eval_all_constraints(m_, C, P, &ch, &cons);
  if (cons.lutre) for (int i = 0; i < r * C->nluts; i++) trace_put(tr, o_fl + 1 + i, cons.lutre[i]);
  long nn = 1L << C->degree_bits;
  E zeta_n = Epow(ch.zeta, nn);
  int nqchunks = C->qdf > 0 ? (P->n_quot + C->qdf - 1) / C->qdf : 0;
  int eqs_ok = 1;
  for (int i = 0; ; i++) {   /* and [ q*(zeta_n-1) == c | (q,c) <- safeZip quotient_evals combined_evals ] */
    if (i == nqchunks && i == r) break;
    if (i >= nqchunks || i >= r) { if (eqs_ok) fail(P2V_ERR_SHAPE, "safeZip: different input lengths (quotient chunks vs alphas)"); break; }
    E c = Eb(0);   /* combineWithPowersOfAlpha :54-56 */
    for (int k = cons.n - 1; k >= 0; k--) c = Eadd(cons.v[k], Escale(ch.alphas[i], c));
    E q = Eb(0);
    int cs = i * C->qdf, ce = cs + C->qdf < P->n_quot ? cs + C->qdf : P->n_quot;
    for (int k = ce - 1; k >= cs; k--) q = Eadd(P->o_quot[k], Emul(zeta_n, q));
    if (tr) { trace_put(tr, o_c + 2 * i, c.a); trace_put(tr, o_c + 2 * i + 1, c.b); trace_put(tr, o_q + 2 * i, q.a); trace_put(tr, o_q + 2 * i + 1, q.b); }
    if (eqs_ok && !Eeq(Emul(q, Esub(zeta_n, Eb(1))), c)) { eqs_ok = 0; if (!tr) break; }
  }
  /* fri_ok: checkFRIProof :358-407 (evaluated only if eqs_ok, unless tracing) */
  int pow_ok = 1;
  {
    F mask = 0; int pb = C->pow_bits;   /* checkProofOfWork :212-216 */
    if (pb > 0 && pb <= 64) mask = (pb == 64 ? ~0ULL : ((1ULL << pb) - 1)) << (64 - pb);
    pow_ok = (ch.pow_response & mask) == 0;
  }
  if (tr) trace_put(tr, o_fl, (F)(eqs_ok | (pow_ok << 1)));
  status = P2V_REJECT;
  if (eqs_ok || tr) {
    int bn1, bn2; E* b1 = fri_batch_this(m_, P, &bn1); E* b2 = fri_batch_next(m_, P, &bn2);
    E y0 = Eb(0), y1 = Eb(0);   /* precomputeReducedOpenings :128-134 */
    for (int i = bn1 - 1; i >= 0; i--) y0 = Eadd(b1[i], Emul(ch.fri_alpha, y0));
    for (int i = bn2 - 1; i >= 0; i--) y1 = Eadd(b2[i], Emul(ch.fri_alpha, y1));
    int fri_status = pow_ok ? P2V_ACCEPT : P2V_REJECT;
    {
      int nq = Q < P->nrounds ? Q : P->nrounds;
      for (int q = 0; q < nq; q++) {
        if (fri_status == P2V_ACCEPT && pow_ok) {   /* the reference's evaluation: errors propagate */
          qres_t res; memset(&res, 0, sizeof res);
          check_query_round(C, P, &ch, y0, y1, arities, nsteps, q, &res, 1);
          if (res.code != 1) fri_status = res.code;
        }
        if (tr) trace_query(C, P, &ch, y0, y1, arities, nsteps, q, tr, o_qin, o_qf, o_qfin);
        if (fri_status != P2V_ACCEPT && !tr) break;
      }
      if (fri_status == P2V_ACCEPT && pow_ok && Q != P->nrounds) fail(P2V_ERR_SHAPE, "safeZipWith: different input lengths (query rounds)");
    }
    status = eqs_ok ? fri_status : P2V_REJECT;
  }
  return status;
}

/* ======================================================================= ABI */
static __thread char g_last[512];
const char* or_last_error(void) { return g_last; }

or_circuit* or_circuit_load(const char* common, size_t clen, const char* vkey, size_t vlen) {
  or_circuit* volatile oc = (or_circuit*)calloc(1, sizeof(or_circuit));
  oj_arena* volatile ja = NULL;
  jmp_buf jb; jmp_buf* saved = g_jb; g_jb = &jb;
  if (setjmp(jb)) { snprintf(g_last, sizeof g_last, "%s", g_msg); oj_arena_free(ja); afree(&oc->c.mem); free(oc); g_jb = saved; return NULL; }
  oj_arena* jl = NULL; oj* cj = oj_parse(common, clen, &jl); ja = jl; if (!cj) fail(P2V_ERR_PARSE, "common: JSON syntax");
  oj* vj = oj_parse(vkey, vlen, &jl); ja = jl; if (!vj) fail(P2V_ERR_PARSE, "vkey: JSON syntax");
  load_circuit(&oc->c, cj, vj);
  oj_arena_free(ja); g_jb = saved;
  return oc;
}
void or_circuit_free(or_circuit* c) { if (c) { afree(&c->c.mem); free(c); } }
/* opt-in plonky2 conventions (P2V_EXT_* of include/p2v.h); 0 = the reference's */
void or_circuit_set_ext(or_circuit* c, unsigned ext) { c->c.ext = ext; }

or_proof* or_proof_load(const char* proof, size_t plen) {
  or_proof* volatile op = (or_proof*)calloc(1, sizeof(or_proof));
  oj_arena* volatile ja = NULL;
  jmp_buf jb; jmp_buf* saved = g_jb; g_jb = &jb;
  if (setjmp(jb)) { snprintf(g_last, sizeof g_last, "%s", g_msg); oj_arena_free(ja); afree(&op->p.mem); free(op); g_jb = saved; return NULL; }
  oj_arena* jl = NULL; oj* pj = oj_parse(proof, plen, &jl); ja = jl; if (!pj) fail(P2V_ERR_PARSE, "proof: JSON syntax");
  load_proof(&op->p, pj);
  oj_arena_free(ja); g_jb = saved;
  return op;
}
void or_proof_free(or_proof* p) { if (p) { afree(&p->p.mem); free(p); } }

/* status of verifyProof; trace (optional) gets P2V_TRACE_WORDS(r,S,Q,L) words.
 * full_trace bit 0 computes every trace value even past a deciding failure; bit 1 sets every
 * gate filter and lookup selector to 1 (parity mode: exposes every constraint program in the
 * combined values C_i of the trace; the status is then meaningless). */
int or_verify(const or_circuit* c, const or_proof* p, uint64_t* trace, int full_trace) {
  int s = verify_impl(&c->c, &p->p, trace, full_trace);
  if (s < 0) snprintf(g_last, sizeof g_last, "%s", g_msg);
  return s;
}

int or_trace_words(const or_circuit* c) {
  jmp_buf jb; jmp_buf* saved = g_jb; g_jb = &jb;
  if (setjmp(jb)) { g_jb = saved; return -1; }
  int ar[64]; int S = expand_strategy(&c->c, ar);
  g_jb = saved;
  return P2V_TRACE_WORDS(c->c.r, S, c->c.nqueries, c->c.nluts);
}

/* helpers exposed for unit tests */
void or_poseidon(uint64_t* st) { or_permutation(st); }
void or_compress(const uint64_t* x, const uint64_t* y, uint64_t* out) { compress(x, y, out); }
uint64_t or_subgroup_gen(int k) { jmp_buf jb; jmp_buf* s = g_jb; g_jb = &jb; if (setjmp(jb)) { g_jb = s; return 0; } F r = subgroup_gen(k); g_jb = s; return r; }
uint64_t or_fmul(uint64_t a, uint64_t b) { return fmul(a, b); }
uint64_t or_finv(uint64_t a) { return finv(a); }

/* gate-level evaluation for parity tests: evaluates the unfiltered constraints of one
 * gate string on given F^2 wires / constants / PI hash. Returns #constraints or <0. */
int or_eval_gate(const char* gate_str, const uint64_t* wires, int nwires, const uint64_t* consts, int nconsts,
                 const uint64_t* pih, uint64_t* out, int maxout) {
  arena m = {0};
  jmp_buf jb; jmp_buf* saved = g_jb; g_jb = &jb;
  if (setjmp(jb)) { snprintf(g_last, sizeof g_last, "%s", g_msg); afree(&m); g_jb = saved; return g_code; }
  gate_t g = parse_gate(gate_str, &m);
  evars_t V = { NULL, 0, NULL, 0, (const E*)consts, nconsts, (const E*)wires, nwires, pih };
  clist l = {0}; l.m = &m;
  gate_constraints(&g, &V, &l);
  int n = l.n < maxout ? l.n : maxout;
  memcpy(out, l.v, (size_t)n * sizeof(E));
  int total = l.n;
  afree(&m); g_jb = saved;
  return total;
}
int or_gate_kind(const char* gate_str) { arena m = {0}; gate_t g = parse_gate(gate_str, &m); afree(&m); return g.kind; }

/* threaded CPU baseline: verify n proofs with `threads` pthreads; returns #accepted */
#include <pthread.h>
typedef struct { const or_circuit* c; or_proof** ps; long n; int8_t* res; long next; pthread_mutex_t mu; } pool_t;
static void* worker(void* arg) {
  pool_t* pl = (pool_t*)arg;
  for (;;) {
    pthread_mutex_lock(&pl->mu); long i = pl->next++; pthread_mutex_unlock(&pl->mu);
    if (i >= pl->n) break;
    pl->res[i] = (int8_t)or_verify(pl->c, pl->ps[i], NULL, 0);
  }
  return NULL;
}
long or_verify_many(const or_circuit* c, or_proof** ps, long n, int8_t* res, int threads) {
  pool_t pl = { c, ps, n, res, 0, PTHREAD_MUTEX_INITIALIZER };
  if (threads < 1) threads = 1;
  pthread_t th[256]; if (threads > 256) threads = 256;
  for (int t = 0; t < threads; t++) pthread_create(&th[t], NULL, worker, &pl);
  for (int t = 0; t < threads; t++) pthread_join(th[t], NULL);
  long acc = 0; for (long i = 0; i < n; i++) acc += res[i] == 1;
  return acc;
}
