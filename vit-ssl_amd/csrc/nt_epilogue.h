// The fused epilogues of the NT GEMM family (csrc/gemm_nt.hip): launch parameters, the table that says what each epilogue is,
// the vector-memory counts derived from it, the GELU table, the wave's LDS window and nt_epilogue itself.
#pragma once
#include "../../include/vitssl_droppath.h"
#include "../../include/vitssl_layerscale.h"
#include "common.h"

namespace {

struct NtParams {
  const bf16_t* A;
  const bf16_t* B;
  long long M;
  int N, K;
  const float* bias;
  const void* aux;
  void* out0;
  void* out1;
  float* colsum;
  float* workspace;          // slot rows of the column sums (caller's, vitssl_gemm_t.workspace)
  int64_t workspace_floats;
  DropKey dk;
  int drop_on;
  vitssl_embed_t embed;
  int tiles_m, tiles_n;
  int group_n;   // tile columns per raster group (their B panels stay L2-resident)
  int k_chunk;   // split-K: K elements per blockIdx.y slice (0 = no split)
  int stagger;   // ping-pong kernel: estimated time of one output tile in 100 MHz ticks (0 = no start-up stagger)
  int esz;       // operand element size in bytes: 2 = bf16, 1 = fp8 e4m3 (ping-pong kernel only)
  const float* alpha;   // fp8 operands: device scalar multiplied into the accumulators (product of the dequantisation scales), or NULL
  void* out2;    // fp8 operands: optional e4m3 image of out1 (EPI_GELU) / of out0 (EPI_DGELU) = the next GEMM's A operand, or NULL
  const float* alpha2;  // second device scalar multiplied into the accumulators (1 / scale of a scaled gradient operand), or NULL
  const float* qscale;  // device scalar the values are multiplied by before they are quantised into out2 (NULL = 1)
  float* qamax;         // device slot that receives max |value| written to out2, before scaling (atomic max; NULL = none)
  const float* rowscale;   // EPI_RESID_ROWS: the branch of row m is multiplied by rowscale[m / rows_per_group] (include/vitssl_droppath.h)
  unsigned rows_per_group;
  const float* colscale;   // EPI_RESID_LS: the branch of column n is multiplied by colscale[n] (LayerScale, include/vitssl_layerscale.h);
                           // rowscale may be NULL there (no drop path) and out1, if given, receives the bf16 image of the branch
#ifdef VITSSL_NT_STAMPS
  unsigned long long* stamps;   // diagnostic build only (tools/nt_stamps.py): [2: 100 MHz ticks, shader clocks][wg][2 wave groups][16 rounds][4]
#endif
};

// ---- what an epilogue is ---------------------------------------------------------------------------------------
// internal epilogue: fp32 output accumulated with atomics by the split-K slices (out0 is
// zeroed by the launcher; slice 0 adds the bias)
constexpr int EPI_F32_SPLITK = 100;
// internal epilogue: VITSSL_EPI_RESID with a per-row scale of the branch (drop path, vitssl_gemm_bf16_nt_rows).  An epilogue id
// of its own, so that the kernels of the plain residual launch are the instantiations they were.
constexpr int EPI_RESID_ROWS = 101;
// internal epilogue: VITSSL_EPI_RESID with a per-column scale of the branch (LayerScale, vitssl_gemm_bf16_nt_ls), an optional
// per-row scale and an optional bf16 image of the branch before both scales.  Again an id of its own.
constexpr int EPI_RESID_LS = 102;

enum NtOut1 { OUT1_NONE, OUT1_REQUIRED, OUT1_OPTIONAL };
struct NtEpiFacts {
  int out0_esz;      // element size of out0 in bytes
  bool windowed;     // out0 / out1 / aux move through the branch-free row windows of nt_epilogue, where every lane's access is issued and
                     // can be counted (the descriptor drops what is out of range); false = plain addressing / atomics under a bounds test
  NtOut1 out1;       // the second bf16 image
  int aux_esz;       // element size of aux, the operand the epilogue reads (0 = none)
  bool colsum, fp8;  // column sums allowed (the epilogues that produce a gradient operand: bias gradients); built for fp8 operands
  int q8_of;         // fp8 operands: the output whose e4m3 image out2 may be written, and may then replace it (-1 = none, 0 = out0, 1 = out1)
  bool drops, resid; // uses the dropout stream; adds the branch to the fp32 residual stream in aux
  int stagger_bit;   // the VITSSL_EPI_* bit of VITSSL_NT_STAGGER_EPIS it staggers by (the rows / LayerScale forms stagger as the residual does)
  float epi_us;      // launch_pp's estimate of one uncontended epilogue
};
constexpr NtEpiFacts nt_epi(int epi) {
  switch (epi) {
    //                                  out0 windowed out1         aux colsum fp8   q8_of drops resid  stagger_bit       epi_us
    case VITSSL_EPI_BF16:  return NtEpiFacts{2, true,  OUT1_NONE,     0, true,  true,  -1, false, false, VITSSL_EPI_BF16,  2.f};
    case VITSSL_EPI_F32:   return NtEpiFacts{4, true,  OUT1_NONE,     0, true,  true,  -1, false, false, VITSSL_EPI_F32,   4.f};
    case VITSSL_EPI_GELU:  return NtEpiFacts{2, true,  OUT1_REQUIRED, 0, false, true,   1, true,  false, VITSSL_EPI_GELU,  7.f};   // out0 = g', out1 = a
    case VITSSL_EPI_RESID: return NtEpiFacts{4, true,  OUT1_NONE,     4, false, true,  -1, true,  true,  VITSSL_EPI_RESID, 8.f};
    case VITSSL_EPI_DGELU: return NtEpiFacts{2, true,  OUT1_NONE,     2, true,  true,   0, false, false, VITSSL_EPI_DGELU, 5.f};   // aux = g'
    case VITSSL_EPI_EMBED: return NtEpiFacts{4, false, OUT1_NONE,     0, false, false, -1, false, false, VITSSL_EPI_EMBED, 4.f};
    case EPI_F32_SPLITK:   return NtEpiFacts{4, false, OUT1_NONE,     0, false, false, -1, false, false, -1,               4.f};   // never in the ping-pong loop
    case EPI_RESID_ROWS:   return NtEpiFacts{4, true,  OUT1_NONE,     4, false, false, -1, true,  true,  VITSSL_EPI_RESID, 8.f};   // + rowscale
    case EPI_RESID_LS:     return NtEpiFacts{4, true,  OUT1_OPTIONAL, 4, false, false, -1, true,  true,  VITSSL_EPI_RESID, 8.f};   // + colscale, rowscale or NULL; out1 = branch
    default:               return NtEpiFacts{0, false, OUT1_NONE,     0, false, false, -1, false, false, -1,               0.f};   // not an epilogue
  }
}

// Rows of 16 that nt_epilogue walks per group; PREF = the line-shaped form, which requests the operands of group g+1 before group g
// is computed and stored (two groups of operands alive at once: 1 row per group for the residual lines, 2 for g').  The group's
// loads are one memory round trip.  The 224-row tiles (MI = 7: every N = 768 launch of ViT-B, both residual epilogues among them)
// take ONE row per group.  Round 3 measured uneven groups (4 + 3) against that, interleaved: N = K = 768 residual 104 -> 109 us,
// K = 3072 residual 251 -> 247 us, dGELU unchanged -- the phase is bound by bytes, not by round trips (as round 1 found for MI = 8).
template <int EPI, int MI, bool PREF>
constexpr int nt_row_group() {
  return nt_epi(EPI).resid ? (PREF ? 1 : (MI % 2 == 0 ? 2 : 1)) : EPI == VITSSL_EPI_DGELU ? (PREF ? 2 : (MI % 4 == 0 ? 4 : 2)) : 4;
}

// Vector-memory instructions per wave that nt_epilogue is CERTAIN to issue for one row tile (16 rows x the wave's 64 columns): the
// loads of aux plus the stores of out0 / out1 / out2.  An image of e-byte elements is e wave-instructions of 16 bytes per lane and
// row tile.  The main loops wait on these counts: vector-memory operations retire in issue order, so "at most <the epilogue's
// operations> still in flight" implies that the staging DMA issued before the epilogue has landed, without waiting for the stores
// themselves.  So a count must be a LOWER bound (a smaller one only waits longer; a larger one would let the next K-tile read a
// staging unit that has not landed): only windowed accesses count, an optional image counts nothing, and with fp8 operands the
// output that its e4m3 image may replace at launch time (the bf16 `a` of GELU, the bf16 dGELU image) counts as that image: 1.
// The narrower store forms (N not a multiple of 8) issue more instructions, never fewer.
template <int EPI, bool F8>
constexpr int nt_epi_row_ops(bool stores_only) {
  constexpr NtEpiFacts E = nt_epi(EPI);
  if (!E.windowed) return 0;
  const int out0 = (F8 && E.q8_of == 0) ? 1 : E.out0_esz;
  const int out1 = E.out1 != OUT1_REQUIRED ? 0 : (F8 && E.q8_of == 1) ? 1 : 2;
  return (stores_only ? 0 : E.aux_esz) + out0 + out1;
}
// ping-pong kernel: the whole epilogue of a wave tile of MI row tiles
template <int EPI, int MI, bool F8>
constexpr int nt_epi_vmem_ops() { return nt_epi_row_ops<EPI, F8>(false) * MI; }
// gemm_nt_kernel (bf16 operands): the stores of the last row group of a 128-row wave tile; kept for the 96- and 112-row tiles,
// whose whole epilogue still issues more (static_assert in the kernel)
template <int EPI>
constexpr int nt_epi_tail_stores() { return nt_epi_row_ops<EPI, false>(true) * nt_row_group<EPI, 8, false>(); }
// the hand-counted literals these derivations replaced, per row tile with bf16 / fp8 operands, and the tail, for every instantiation
template <int EPI, int MI>
constexpr bool nt_counts_are(int bf, int f8, int tail) {
  return nt_epi_vmem_ops<EPI, MI, false>() == bf * MI && (!nt_epi(EPI).fp8 || nt_epi_vmem_ops<EPI, MI, true>() == f8 * MI) &&
         nt_epi_tail_stores<EPI>() == tail;
}
template <int MI>
constexpr bool nt_counts_are_as_written() {
  return nt_counts_are<VITSSL_EPI_BF16, MI>(2, 2, 8) && nt_counts_are<VITSSL_EPI_GELU, MI>(4, 3, 16) && nt_counts_are<VITSSL_EPI_DGELU, MI>(4, 3, 8) &&
         nt_counts_are<VITSSL_EPI_F32, MI>(4, 4, 16) && nt_counts_are<VITSSL_EPI_RESID, MI>(8, 8, 8) && nt_counts_are<EPI_RESID_ROWS, MI>(8, 8, 8) &&
         nt_counts_are<EPI_RESID_LS, MI>(8, 8, 8) && nt_counts_are<VITSSL_EPI_EMBED, MI>(0, 0, 0) && nt_counts_are<EPI_F32_SPLITK, MI>(0, 0, 0);
}
static_assert(nt_counts_are_as_written<6>() && nt_counts_are_as_written<7>() && nt_counts_are_as_written<8>(), "epilogue vmem counts");


// ---- GELU by table (EPI_GELU of the ping-pong kernel) ---------------------------------------------------------
// The epilogue evaluates gelu / gelu' on the pre-activation ROUNDED TO bf16 (the reference's autocast stores that tensor
// in bf16, feed_forward.py:26-27), i.e. on one of 65536 inputs, and writes two bf16 results.  For 2^-14 <= |u| < 16
// (18 binades x 128 mantissas x 2 signs = 4608 inputs, all but ~1e-4 of the elements) the pair
// (bf16(s gelu(u)), bf16(s gelu'(u))), s = dropout scale, is read from an 18 KiB table in the LDS the staging buffers
// leave free; the workgroup fills it once per launch with gelu_both_scaled, so every entry is bit-identical to what the
// arithmetic path produces for that input.  A 4-element group with any lane outside the range (wave-uniform test) is
// redone with the arithmetic.  Why: the arithmetic is ~60 VALU cycles per element of an epilogue that is VALU-issue
// bound (tools/probes/valu_rates.hip: v_exp / v_rcp 8.2 cycles, packed fp32 4.8 per pair); the lookup is ~25 cycles of
// index arithmetic plus one ds_read_b32 on the otherwise idle LDS pipe (8 cycles per wave-instruction per CU with random
// addresses).
constexpr int GLUT_E_LO = 127 - 14;                       // bf16 exponent field of 2^-14
constexpr int GLUT_BINADES = 18;                          // ... up to [8, 16)
constexpr int GLUT_ENTRIES = GLUT_BINADES * 128 * 2;      // (magnitude index, sign)
constexpr int GLUT_BYTES = GLUT_ENTRIES * 4;
constexpr unsigned GLUT_LO8 = (unsigned)GLUT_E_LO << 10;  // magnitude part of the byte address: (h & 0x7fff) << 3
constexpr unsigned GLUT_HI8 = (unsigned)(GLUT_E_LO + GLUT_BINADES) << 10;

// Table addressing.  Entry (magnitude index m, sign s) of bf16 pattern h sits at byte (2 m + s) * 4 = rot16(h, 1) * 4 (relative to
// table base - GLUT_LO8): both halves of a packed pair are rotated by two packed 16-bit instructions, an SDWA shift per element
// turns a half into its byte address, and the range test of a 4-element group is three packed 16-bit instructions on the
// rotated words (16 instructions per group less than shift / and / min / or per element).  A lane outside the table's range
// reads staging bytes or beyond the workgroup's LDS (reads return 0 there): its group is redone arithmetically.
__device__ __forceinline__ unsigned glut_rot2(unsigned w) {
  unsigned t, r;
  asm("v_pk_lshrrev_b16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(t) : "v"(w));            // sign of each half (the inline constant serves both)
  asm("v_pk_mad_u16 %0, %1, 2, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(w), "v"(t));     // (h << 1) + sign, modulo 2^16
  return r;
}
__device__ __forceinline__ void glut_addr2(unsigned r, unsigned& a0, unsigned& a1) {
  asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(a0) : "v"(r));
  asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(a1) : "v"(r));
}
// true when any of the four rotated patterns lies outside [2 LO, 2 HI): d = r - 2 LO (modulo 2^16) must be <= 2 (HI - LO) - 1
__device__ __forceinline__ bool glut_out_of_range(unsigned r01, unsigned r23) {
  const unsigned lo2 = ((unsigned)GLUT_E_LO << 8) * 0x10001u, span = ((unsigned)(GLUT_BINADES << 8) - 1u) * 0x10001u;
  unsigned d01, d23, dm, e;
  asm("v_pk_sub_u16 %0, %1, %2" : "=v"(d01) : "v"(r01), "s"(lo2));
  asm("v_pk_sub_u16 %0, %1, %2" : "=v"(d23) : "v"(r23), "s"(lo2));
  asm("v_pk_max_u16 %0, %1, %2" : "=v"(dm) : "v"(d01), "v"(d23));
  asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(e) : "v"(dm), "s"(span));
  return e != 0;
}
// plain LDS loads (the compiler counts them): checked in the .s that no vmcnt wait is attached to them -- the operand DMA in
// flight during the epilogue writes other LDS bytes, but hipcc cannot always prove that (cdna guide, "three .s-level traps")
// (Addressed as a raw LDS offset: through the `smem` symbol hipcc emits one `v_add_u32 v, 0, v` per lookup that it does not fold.
// The kernel has no static LDS, so its dynamic LDS starts at offset 0; the kernel traps at entry if that ever stops being true.)
template <int OFF>
__device__ __forceinline__ unsigned glut_read(const char* smem, unsigned a) {
  (void)smem;
  return *(const __attribute__((address_space(3))) unsigned*)(unsigned long long)(a + (unsigned)OFF);
}

// ---- the wave's LDS window (line-shaped form) -------------------------------------------------------------------
// Line-shaped accesses go through 2 KiB of LDS private to the wave, so that an instruction's 64 lanes cover 8 rows x 128
// CONTIGUOUS bytes with adjacent lanes on adjacent addresses.  tools/probes/store_patterns.hip: a CU stores 55 GB/s in the
// accumulator layout (adjacent lanes = adjacent ROWS, 16 bytes each: every lane is its own request) and 183-190 GB/s once four
// or more adjacent lanes are contiguous.  A 16-row tile of an image is 16 rows x 128 bytes
// (64 bf16 columns, or the 32 fp32 columns of a pair).  It is written in the accumulator layout (lane (m, c) = row m, 8- or
// 16-byte chunk), with the chunk position XORed by the row so the writes spread over the banks, and read back as lane
// (rho, kappa) = row rho (+8 for the second read), 16-byte chunk kappa: 8 lanes = one 128-byte line.  The loads take the same
// path backwards.
struct NtWindow {
  char* xs;
  unsigned tw16, tr16a, tw32, tr32a;   // this lane's byte offsets in the accumulator layout (tw) and as lines (tr), formed in nt_epilogue
  // a row tile of a bf16 image, accumulator layout w[jp][h] -> its lines of rows 0-7 and 8-15
  __device__ __forceinline__ void lines_of_bf16(const u32x2 (&w)[2][2], u32x4& s1, u32x4& s2) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) *(u32x2*)(xs + (tw16 ^ (unsigned)(32 * j))) = w[j >> 1][j & 1];
    s1 = *(const u32x4*)(xs + tr16a);
    s2 = *(const u32x4*)(xs + ((tr16a + 1024u) ^ 64u));
  }
  // ... and back: the two lines in (the window holds the whole row tile), then tile j = 2 jp + h in the accumulator layout out
  __device__ __forceinline__ void put_lines_bf16(const u32x4& s1, const u32x4& s2) const {
    *(u32x4*)(xs + tr16a) = s1;
    *(u32x4*)(xs + ((tr16a + 1024u) ^ 64u)) = s2;
  }
  __device__ __forceinline__ u32x2 bf16_of_lines(int j) const { return *(const u32x2*)(xs + (tw16 ^ (unsigned)(32 * j))); }
  // one pair (32 columns) of a row tile of an fp32 image, accumulator layout -> its lines of rows 0-7 and 8-15
  __device__ __forceinline__ void lines_of_f32(const f32x4& v0, const f32x4& v1, u32x4& s1, u32x4& s2) const {
    *(f32x4*)(xs + tw32) = v0;
    *(f32x4*)(xs + (tw32 ^ 64u)) = v1;
    s1 = *(const u32x4*)(xs + tr32a);
    s2 = *(const u32x4*)(xs + tr32a + 1024);
  }
  // ... and back, in place
  __device__ __forceinline__ void f32_of_lines(f32x4& v0, f32x4& v1) const {
    *(f32x4*)(xs + tr32a) = v0;
    *(f32x4*)(xs + tr32a + 1024) = v1;
    v0 = *(const f32x4*)(xs + tw32);
    v1 = *(const f32x4*)(xs + (tw32 ^ 64u));
  }
};

__device__ __forceinline__ float amax4(float a, float b, float c, float d) { return fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d))); }

// Fused epilogue of one 128x64 wave tile (shared by both main-loop variants).
template <int EPI, typename CFG, bool Q8 = false, int GLUT_OFF = -1, bool TLS = false>
__device__ __forceinline__ void nt_epilogue(const NtParams& p, f32x4 (&acc)[4][CFG::MI], const long long m0, const int n0,
                                            const int wm, const int wn, const int lane_in, const char* lds = nullptr, char* xs = nullptr) {
  constexpr int MI = CFG::MI;
  constexpr NtEpiFacts E = nt_epi(EPI);
  constexpr bool LS = EPI == EPI_RESID_LS;
  // the lane-only address constants below are re-derived in every epilogue: hoisted out of the tile loop they stay live through
  // the K loop, and the 256-row kernels (128 accumulator registers) then spill K-loop state into scratch
  int lane = lane_in;
  if (TLS) asm volatile("" : "+v"(lane));
  // TLS: xs = this wave's private 2 KiB of LDS (ping-pong kernel: its own B1 staging slots of the buffer that is not being
  // refilled, see the kernel) and N is a multiple of 8; otherwise the stores leave in the accumulator layout
  // GLUT_OFF >= 0: LDS byte offset of the GELU table minus GLUT_LO8 (the ds_read's immediate)
  constexpr bool GLUT = EPI == VITSSL_EPI_GELU && GLUT_OFF >= 0;
  // fp8 operands: the table's entries are (bf16 s gelu'(u)) | (e4m3(s gelu(u) qs) << 16) -- the e4m3 byte is quantised from
  // the fp32 value when the table is built, exactly as the arithmetic path does per element -- and serve launches that
  // write the g' image and the e4m3 image only (no bf16 `a`, no amax: what engine.EncoderStack asks for); launch-uniform
  const bool glut_on = GLUT && (!Q8 || (p.out1 == nullptr && p.qamax == nullptr));
  constexpr bool CS = E.colsum, DROPS = E.drops;   // (the entry point rejects column sums elsewhere)
  float csum[4][4];
  if (CS && p.colsum) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) csum[j][r] = 0.f;
  }
  // ================================================================== 1. geometry
  // All global traffic of the epilogue goes through raw buffer instructions on a window
  // that starts at the tile's first row: rows past M fall outside num_records and columns
  // past N get the out-of-range offset, so loads return 0 and stores are dropped WITHOUT a
  // branch.  That lets every residual / g' load of a 64-column half be issued back to back
  // before the first use (the branchy form waited for each 16-byte load in turn: 32
  // dependent HBM round trips per wave, measured +65 us on the N = K = 768 projection).
  const int g4 = lane >> 4;                       // lane group = 16-lane row of the wave
  // bf16 images: tile columns (j, j+1) exchange halves between lane rows (g, g^1) with
  // v_permlane16_swap so that every lane moves 16 contiguous bytes (8 columns).
  const bool wide = TLS || (p.N & 7) == 0;
  constexpr unsigned OOB = 0x80000000u;
  const long long rows_left = p.M - m0;
  auto window = [&](const void* base, int elt) {
    const unsigned long long bytes = (unsigned long long)rows_left * (unsigned long long)p.N * (unsigned)elt;
    const unsigned rec = bytes > 0x80000000ull ? 0x80000000u : (unsigned)bytes;
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + m0 * p.N * elt), 0, (int)rec, 0x00020000);
  };
  const unsigned row_l = (unsigned)(wm * CFG::WROWS + (lane & 15));      // + 16 i : row inside the tile
  const unsigned un = (unsigned)p.N;
  const int odd = g4 & 1;

  // accumulator layout: byte offset of this lane's 16-byte piece of the bf16 image (wide form), row i, pair jp; ... of its piece at column n
  auto off_bf16_wide = [&](int i, int jp) -> unsigned {
    const int n = n0 + wn * 64 + (2 * jp + odd) * 16 + 4 * (g4 - odd);
    return n < p.N ? ((row_l + 16u * i) * un + (unsigned)n) * 2u : OOB;
  };
  auto off_elem = [&](int i, int n, unsigned elt) -> unsigned { return n < p.N ? ((row_l + 16u * i) * un + (unsigned)n) * elt : OOB; };
  // line layout (TLS, through the wave's LDS window): lane (rho, kappa) = row rho (+ 8) of the row tile, 16-byte chunk kappa
  constexpr bool tls = TLS;
  const int tm = lane & 15, trho = lane >> 3, tkap = lane & 7;
  // bf16: this lane's 8-byte chunk of tile j is chunk (4j + c) ^ 2 (m >> 1) of row m: tile 0's offset, tile j's = that ^ 32 j
  const unsigned tw16 = (unsigned)(tm * 128 + ((g4 ^ (2 * (tm >> 1))) << 3));
  const unsigned tr16a = (unsigned)(trho * 128 + ((tkap ^ (trho >> 1)) << 4));      // rows 0-7: 16-byte chunk kappa; rows 8-15: (+1024) ^ 64
  // fp32: 16-byte chunk (4h + c) ^ (m & 7) of the pair's 128-byte row: tile 0's offset, tile 1's = that ^ 64
  const unsigned tw32 = (unsigned)(tm * 128 + ((g4 ^ (tm & 7)) << 4));
  const unsigned tr32a = (unsigned)(trho * 128 + ((tkap ^ trho) << 4));              // rows 8-15: + 1024 ((rho + 8) & 7 == rho & 7)
  const NtWindow win{xs, tw16, tr16a, tw32, tr32a};
  const unsigned trow = (unsigned)(wm * CFG::WROWS + trho);                // + 16 i (+ 8): row inside the tile
  // lane part of the offsets (row trho of tile 0; out-of-range columns get the sentinel, which stays out of range when the
  // wave-uniform row term below is added: that term is < 2^31); the row term is scalar arithmetic
  const int tn16 = n0 + wn * 64 + 8 * tkap;
  const unsigned tb16 = tn16 < p.N ? (trow * un + (unsigned)tn16) * 2u : OOB;
  auto off_line16 = [&](int i, int half) -> unsigned { return tb16 + (unsigned)(16 * i + 8 * half) * (un * 2u); };   // bf16 image: 8 columns per lane
  auto off_line32 = [&](int i, int jp, int half) -> unsigned {              // fp32 image: 4 columns per lane
    const int n = n0 + wn * 64 + 32 * jp + 4 * tkap;
    const unsigned b = n < p.N ? (trow * un + (unsigned)n) * 4u : OOB;
    return b + (unsigned)(16 * i + 8 * half) * (un * 4u);
  };
  // Column bookkeeping of this wave's 64 columns: pair jp covers tiles (2jp, 2jp+1), half h
  // of a pair is one 16-column tile; a lane owns 4 consecutive columns of each (filled with the bias below).
  int nn[2][2];
  bool okn[2][2];
  // ================================================================== 2. stores
  auto pack_pair = [&](const u32x2& w0, const u32x2& w1) -> u32x4 {
    // after the swap: even lane rows hold tile 2jp cols 4g .. 4g+7, odd rows tile 2jp+1 cols 4(g-1) .. 4(g-1)+7
    auto lo = __builtin_amdgcn_permlane16_swap(w0[0], w1[0], false, false);
    auto hi = __builtin_amdgcn_permlane16_swap(w0[1], w1[1], false, false);
    return u32x4{lo[0], hi[0], lo[1], hi[1]};
  };
  // one row tile of a bf16 image: w[jp][h]; AUXV = cache policy of the stores (buffer aux bits: 1 = sc0, 2 = nt, 16 = sc1)
  auto store_bf16_row = [&](__amdgpu_buffer_rsrc_t rs, int i, const u32x2 (&w)[2][2], auto aux_c) {
    constexpr int AUXV = decltype(aux_c)::value;
    if (tls) {
      u32x4 s1, s2;
      win.lines_of_bf16(w, s1, s2);
      __builtin_amdgcn_raw_buffer_store_b128(s1, rs, off_line16(i, 0), 0, AUXV);
      __builtin_amdgcn_raw_buffer_store_b128(s2, rs, off_line16(i, 1), 0, AUXV);
    } else if (wide) {
      const u32x4 a = pack_pair(w[0][0], w[0][1]), b = pack_pair(w[1][0], w[1][1]);
      __builtin_amdgcn_raw_buffer_store_b128(a, rs, off_bf16_wide(i, 0), 0, AUXV);
      __builtin_amdgcn_raw_buffer_store_b128(b, rs, off_bf16_wide(i, 1), 0, AUXV);
    } else {
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int na = n0 + wn * 64 + (2 * jp) * 16 + 4 * g4;
        __builtin_amdgcn_raw_buffer_store_b64(w[jp][0], rs, off_elem(i, na, 2u), 0, AUXV);
        __builtin_amdgcn_raw_buffer_store_b64(w[jp][1], rs, off_elem(i, na + 16, 2u), 0, AUXV);
      }
    }
  };
  // one pair (32 columns) of a row tile of an fp32 image.  Residual-stream stores (read next by a different kernel) are
  // non-temporal (aux 2): interleaved A/B on MI355X, out-projection shape M = 50176, N = K = 768: 116 -> 97 us; neutral at K = 3072
  constexpr int F32_AUX = E.resid ? 2 : 0;
  auto store_f32_pair = [&](__amdgpu_buffer_rsrc_t rs, int i, int jp, const f32x4& v0, const f32x4& v1, const int (&nnp)[2]) {
    if (tls) {
      u32x4 s1, s2;
      win.lines_of_f32(v0, v1, s1, s2);
      __builtin_amdgcn_raw_buffer_store_b128(s1, rs, off_line32(i, jp, 0), 0, F32_AUX);
      __builtin_amdgcn_raw_buffer_store_b128(s2, rs, off_line32(i, jp, 1), 0, F32_AUX);
    } else {
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v0), rs, off_elem(i, nnp[0], 4u), 0, F32_AUX);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v1), rs, off_elem(i, nnp[1], 4u), 0, F32_AUX);
    }
  };
  // one row tile of the e4m3 image: out_q[jp][h] = this lane's four columns of tile 2jp + h
  auto store_fp8_row = [&](__amdgpu_buffer_rsrc_t rs, int i, const unsigned (&out_q)[2][2]) {
    if ((p.N & 15) == 0) {
      // The row's 64 bytes: dword t*4 + g lives in lane row g as out_q of tile t.  A 4x4 transpose over the
      // four lane rows (permlane32_swap exchanges the wave halves, permlane16_swap odd / even rows) leaves
      // lane row g with dwords 4g .. 4g+3 = 16 contiguous bytes: one store instruction per row tile.
      auto s02 = __builtin_amdgcn_permlane32_swap(out_q[0][0], out_q[1][0], false, false);
      auto s13 = __builtin_amdgcn_permlane32_swap(out_q[0][1], out_q[1][1], false, false);
      auto e = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
      auto f = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
      if (tls) {
        // 16 rows x 64 bytes through the LDS window: written as lane (m, c) -> row m, chunk c ^ ((m >> 1) & 3), read as
        // lane (rho = lane >> 2, kappa = lane & 3): the four lanes of a quad cover one row's 64 contiguous bytes
        *(u32x4*)(xs + tm * 64 + ((g4 ^ ((tm >> 1) & 3)) << 4)) = u32x4{e[0], e[1], f[0], f[1]};
        const int rho4 = lane >> 2, kap4 = lane & 3;
        const u32x4 s8 = *(const u32x4*)(xs + rho4 * 64 + ((kap4 ^ ((rho4 >> 1) & 3)) << 4));
        const int n8 = n0 + wn * 64 + 16 * kap4;
        const unsigned o8 = n8 < p.N ? ((unsigned)(wm * CFG::WROWS + 16 * i + rho4) * un + (unsigned)n8) : OOB;
        __builtin_amdgcn_raw_buffer_store_b128(s8, rs, o8, 0, 0);
      } else {
        const int n = n0 + wn * 64 + 16 * g4;
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{e[0], e[1], f[0], f[1]}, rs, off_elem(i, n, 1u), 0, 0);
      }
    } else {
#pragma unroll
      for (int jp = 0; jp < 2; ++jp)
#pragma unroll
        for (int h = 0; h < 2; ++h) __builtin_amdgcn_raw_buffer_store_b32(out_q[jp][h], rs, off_elem(i, nn[jp][h], 1u), 0, 0);
    }
  };

  // ================================================================== 3. operands: the windows of the buffers nt_epi(EPI) names, ...
  __amdgpu_buffer_rsrc_t rsOut0, rsOut1, rsOut2, rsAux;
  constexpr bool Q8EPI = Q8 && E.q8_of >= 0;
  const bool q8 = Q8EPI && p.out2 != nullptr;
  if (q8) rsOut2 = window(p.out2, 1);
  const float qs = (Q8EPI && p.qscale) ? *p.qscale : 1.0f;
  float qmax = 0.f;                               // running max |value| of this lane's share of the e4m3 image
  if constexpr (E.windowed) rsOut0 = window(p.out0, E.out0_esz);
  if constexpr (E.out1 != OUT1_NONE) {
    if (E.out1 == OUT1_REQUIRED || p.out1) rsOut1 = window(p.out1, 2);         // launch-uniform
  }
  if constexpr (E.aux_esz != 0) rsAux = window(p.aux, E.aux_esz);

  f32x4 bias4[2][2];
  f32x4 gam4[2][2];        // RESID_LS: colscale of this lane's 16 columns, loaded once per column tile like the bias
  // dropout stream (common.h): the state word of group g = row * N/4 + col/4 is g * C0 + k0 = (row term) + (column term);
  // the row term advances by a launch constant per 16-row tile, the column terms are four lane constants
  unsigned a0col[2][2];
  const unsigned a0rowstep = 16u * (unsigned)(p.N >> 2) * DROP_C0;
  unsigned a0row = 0;
  if (DROPS && p.drop_on)
    a0row = drop_a0(p.dk, (unsigned)(m0 + wm * CFG::WROWS + (lane & 15)) * (unsigned)(p.N >> 2));
  // GELU: the dropout scale is folded into the two constants of gelu_both_scaled
  const float gelu_hs = (DROPS && p.drop_on) ? 0.5f * p.dk.scale : 0.5f;
  const float gelu_cs = (DROPS && p.drop_on) ? 0.3989422804014327f * p.dk.scale : 0.3989422804014327f;
#pragma unroll
  for (int jp = 0; jp < 2; ++jp)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      nn[jp][h] = n0 + wn * 64 + (2 * jp + h) * 16 + 4 * g4;
      a0col[jp][h] = (unsigned)(nn[jp][h] >> 2) * DROP_C0;
      okn[jp][h] = nn[jp][h] < p.N;
      bias4[jp][h] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p.bias && (EPI != EPI_F32_SPLITK || blockIdx.y == 0) && okn[jp][h]) bias4[jp][h] = *(const f32x4*)(p.bias + nn[jp][h]);
      if constexpr (LS) {
        gam4[jp][h] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (okn[jp][h]) gam4[jp][h] = *(const f32x4*)(p.colscale + nn[jp][h]);
      }
    }

  // Rows are walked in groups (nt_row_group); inside a group the loop order is row -> pair, so the two
  // 64-byte halves of every 128-byte output line are stored by consecutive instructions
  // (pair-major order left them half an epilogue apart and the second bf16 image of the GELU
  // epilogue was written at ~3 TB/s).  The residual / g' operands of a whole group are
  // loaded before its first use.
  // Operand prefetch (line-shaped form only): the residual / g' lines of group g+1 are requested BEFORE group g
  // is computed and stored.  The vector-memory counter retires in issue order, so in the plain order (loads of g+1 behind the
  // stores of g) the wait for a group's operands also waited for the previous group's stores to be acknowledged by the L2 --
  // one load round trip plus one store round trip per group, 7 times per tile for the 224-row residual epilogue.
  constexpr bool PREF = TLS && E.aux_esz != 0;
  constexpr int RG = nt_row_group<EPI, MI, PREF>();
  constexpr int NB = PREF ? 2 : 1;
  f32x4 res[NB][RG][2][2];   // RESID: residual stream (line layout until used)
  u32x4 raw[NB][RG][2];      // DGELU, 16-byte form: g' as loaded
  float rsc[NB][RG];         // RESID_ROWS / RESID_LS: the scale of this lane's accumulator row (row tile ig + ii), requested with the group's residual
  auto load_group = [&](const int ig, const int b) {
    const int cnt = MI - ig < RG ? MI - ig : RG;
    if constexpr (EPI == EPI_RESID_ROWS || LS) {
#pragma unroll
      for (int ii = 0; ii < RG; ++ii) {
        if (ii >= cnt) continue;
        if constexpr (LS) rsc[b][ii] = 1.0f;
        if (EPI == EPI_RESID_ROWS || p.rowscale) {    // RESID_LS: launch-uniform, the table is optional
          // rows past M read entry 0 (their stores are dropped); m < M < 2^31 / K, and groups * rows_per_group == M keeps the index inside the table
          const long long mr = m0 + wm * CFG::WROWS + (ig + ii) * 16 + (lane & 15);
          rsc[b][ii] = p.rowscale[mr < p.M ? (unsigned)mr / p.rows_per_group : 0u];
        }
      }
    }
    if constexpr (E.resid) {
#pragma unroll
      for (int ii = 0; ii < RG; ++ii)
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          if (ii >= cnt) continue;
          if (tls) {
            // whole lines (8 rows x 128 bytes per instruction); turned into the accumulator layout through the LDS window at use
            res[b][ii][jp][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsAux, off_line32(ig + ii, jp, 0), 0, 0));
            res[b][ii][jp][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsAux, off_line32(ig + ii, jp, 1), 0, 0));
          } else {
#pragma unroll
            for (int h = 0; h < 2; ++h)
              res[b][ii][jp][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsAux, off_elem(ig + ii, nn[jp][h], 4u), 0, 0));
          }
        }
    }
    if constexpr (EPI == VITSSL_EPI_DGELU) {
      if (wide) {
#pragma unroll
        for (int ii = 0; ii < RG; ++ii) {
          if (ii >= cnt) continue;
          if (tls) {
            raw[b][ii][0] = __builtin_amdgcn_raw_buffer_load_b128(rsAux, off_line16(ig + ii, 0), 0, 0);    // rows 0-7 of the row tile, whole lines
            raw[b][ii][1] = __builtin_amdgcn_raw_buffer_load_b128(rsAux, off_line16(ig + ii, 1), 0, 0);    // rows 8-15
          } else {
#pragma unroll
            for (int jp = 0; jp < 2; ++jp) raw[b][ii][jp] = __builtin_amdgcn_raw_buffer_load_b128(rsAux, off_bf16_wide(ig + ii, jp), 0, 0);
          }
        }
      }
    }
  };
  if constexpr (PREF) load_group(0, 0);
#pragma unroll
  for (int ig = 0; ig < MI; ig += RG) {
    const int cnt = MI - ig < RG ? MI - ig : RG;      // (a constant once the loop is unrolled)
    const int gb = PREF ? (ig / RG) & 1 : 0;
    if constexpr (!PREF) load_group(ig, 0);
    else if (ig + RG < MI) load_group(ig + RG, gb ^ 1);
    u32x2 gpre[RG][2][2];    // DGELU: g' in accumulator layout
    if constexpr (EPI == VITSSL_EPI_DGELU) {
      if (wide) {
#pragma unroll
        for (int ii = 0; ii < RG; ++ii)
#pragma unroll
          for (int jp = 0; jp < 2; ++jp) {
            if (ii >= cnt) continue;
            if (tls) {
              if (jp == 0) {                        // (both pairs at once)
                win.put_lines_bf16(raw[gb][ii][0], raw[gb][ii][1]);
#pragma unroll
                for (int j = 0; j < 4; ++j) gpre[ii][j >> 1][j & 1] = win.bf16_of_lines(j);
              }
              continue;
            }
            // inverse of the store shuffle (the swap is an involution)
            auto sa = __builtin_amdgcn_permlane16_swap(raw[gb][ii][jp][0], raw[gb][ii][jp][2], false, false);
            auto sb = __builtin_amdgcn_permlane16_swap(raw[gb][ii][jp][1], raw[gb][ii][jp][3], false, false);
            gpre[ii][jp][0] = u32x2{sa[0], sb[0]};
            gpre[ii][jp][1] = u32x2{sa[1], sb[1]};
          }
      } else {
#pragma unroll
        for (int ii = 0; ii < RG; ++ii)
#pragma unroll
          for (int jp = 0; jp < 2; ++jp)
#pragma unroll
            for (int h = 0; h < 2; ++h)
              if (ii < cnt) gpre[ii][jp][h] = __builtin_amdgcn_raw_buffer_load_b64(rsAux, off_elem(ig + ii, nn[jp][h], 2u), 0, 0);
      }
    }

    // ================================================================ 4. the group's rows: arithmetic by epilogue, then the row's stores
#pragma unroll
    for (int ii = 0; ii < RG; ++ii) {
      if (ii >= cnt) continue;
      const int i = ig + ii;
      const long long m = m0 + wm * CFG::WROWS + i * 16 + (lane & 15);
      const bool okm = m < p.M;
      u32x2 out_a[2][2], out_b[2][2];   // bf16 images of this row, both pairs: stored together below
      unsigned out_q[2][2];             // e4m3 image of out_b (fp8 operand path)
      // GELU by table: the row's 16 lookups are issued first and fly under the dropout-stream arithmetic below
      unsigned gl[16];                  // (bf16 s gelu(u)) | (bf16 s gelu'(u)) << 16 per element: [jp][h][r]
      bool gslow[2][2];                 // wave-uniform: some lane of this group is outside the table's range
      if (GLUT && glut_on) {
#pragma unroll
        for (int jp = 0; jp < 2; ++jp)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f32x4 vv = acc[2 * jp + h][i] + bias4[jp][h];
            const unsigned w0 = pack_bf2(vv[0], vv[1]), w1 = pack_bf2(vv[2], vv[3]);
            const unsigned r01 = glut_rot2(w0), r23 = glut_rot2(w1);
            gslow[jp][h] = __builtin_amdgcn_ballot_w64(glut_out_of_range(r01, r23)) != 0;
            unsigned ad[4];
            glut_addr2(r01, ad[0], ad[1]);
            glut_addr2(r23, ad[2], ad[3]);
            const int q = 8 * jp + 4 * h;
#pragma unroll
            for (int r = 0; r < 4; ++r) gl[q + r] = glut_read<GLUT_OFF>(lds, ad[r]);
          }
      }
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        f32x4 v[2] = {acc[2 * jp][i] + bias4[jp][0], acc[2 * jp + 1][i] + bias4[jp][1]};

        if constexpr (EPI == VITSSL_EPI_BF16) {
          out_a[jp][0] = u32x2{pack_bf2(v[0][0], v[0][1]), pack_bf2(v[0][2], v[0][3])};
          out_a[jp][1] = u32x2{pack_bf2(v[1][0], v[1][1]), pack_bf2(v[1][2], v[1][3])};
        } else if constexpr (EPI == VITSSL_EPI_GELU) {
          // u = bf16(acc + bias) (never stored); out1 = a = keep*scale*gelu(u) feeds the next
          // GEMM; out0 = g' = keep*scale*gelu'(u) is what the backward dGELU epilogue needs.
          // keep masks of each group's two bf16 pairs (0xffff per kept element), ANDed onto the packed outputs
          unsigned km[2][2] = {{0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}};
          u32x2 dw[2] = {u32x2{0u, 0u}, u32x2{0u, 0u}};
          const bool dropping = p.drop_on;
          if (dropping) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              dw[h] = drop_words_a0(p.dk, a0row + (unsigned)i * a0rowstep + a0col[jp][h]);
              km[h][0] = drop_keep_pair(p.dk, dw[h][0]);
              km[h][1] = drop_keep_pair(p.dk, dw[h][1]);
            }
          }
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (GLUT && glut_on && !gslow[jp][h]) {
              const int q = 8 * jp + 4 * h;
              // the low halves of the entries: `a` of the bf16 table, g' of the fp8 one
              const u32x2 lo = u32x2{__builtin_amdgcn_perm(gl[q + 1], gl[q], 0x05040100u) & km[h][0],
                                     __builtin_amdgcn_perm(gl[q + 3], gl[q + 2], 0x05040100u) & km[h][1]};
              if constexpr (!Q8) {
                out_b[jp][h] = lo;
                out_a[jp][h] = u32x2{__builtin_amdgcn_perm(gl[q + 1], gl[q], 0x07060302u) & km[h][0],
                                     __builtin_amdgcn_perm(gl[q + 3], gl[q + 2], 0x07060302u) & km[h][1]};
              } else {
                out_a[jp][h] = lo;
                // the four e4m3 bytes (byte 2 of every entry) and the byte mask of the kept elements
                const unsigned b01 = __builtin_amdgcn_perm(gl[q + 1], gl[q], 0x0c0c0602u), b23 = __builtin_amdgcn_perm(gl[q + 3], gl[q + 2], 0x06020c0cu);
                out_q[jp][h] = (b01 | b23) & __builtin_amdgcn_perm(km[h][1], km[h][0], 0x06040200u);
              }
              continue;
            }
            float y[4], d[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) gelu_both_scaled(round_bf(v[h][r]), gelu_hs, gelu_cs, y[r], d[r]);
            out_b[jp][h] = u32x2{pack_bf2(y[0], y[1]) & km[h][0], pack_bf2(y[2], y[3]) & km[h][1]};
            out_a[jp][h] = u32x2{pack_bf2(d[0], d[1]) & km[h][0], pack_bf2(d[2], d[3]) & km[h][1]};
            if constexpr (Q8) {
              if (dropping) {
                bool keep[4];
                drop_keep4(p.dk, dw[h], keep);
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = keep[r] ? y[r] : 0.f;
              }
              out_q[jp][h] = pack_fp8x4(y[0] * qs, y[1] * qs, y[2] * qs, y[3] * qs);
              if (okm && okn[jp][h]) qmax = fmaxf(qmax, amax4(y[0], y[1], y[2], y[3]));
            }
          }
        } else if constexpr (EPI == VITSSL_EPI_DGELU) {
          // du = acc * g'  (g' already carries the dropout mask and its scale)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const u32x2 gpv = gpre[ii][jp][h];
            v[h][0] *= bf_lo(gpv[0]);
            v[h][1] *= bf_hi(gpv[0]);
            v[h][2] *= bf_lo(gpv[1]);
            v[h][3] *= bf_hi(gpv[1]);
            out_a[jp][h] = u32x2{pack_bf2(v[h][0], v[h][1]), pack_bf2(v[h][2], v[h][3])};
            if constexpr (Q8) {
              out_q[jp][h] = pack_fp8x4(v[h][0] * qs, v[h][1] * qs, v[h][2] * qs, v[h][3] * qs);
              if (okm && okn[jp][h]) qmax = fmaxf(qmax, amax4(v[h][0], v[h][1], v[h][2], v[h][3]));
            }
          }
        } else if constexpr (EPI == EPI_F32_SPLITK) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (!(okm && okn[jp][h])) continue;
            float* o = (float*)p.out0 + m * p.N + nn[jp][h];
#pragma unroll
            for (int r = 0; r < 4; ++r) unsafeAtomicAdd(o + r, v[h][r]);
          }
        } else if constexpr (EPI == VITSSL_EPI_F32) {
          store_f32_pair(rsOut0, i, jp, v[0], v[1], nn[jp]);
        } else if constexpr (E.resid) {
          // the pair's residual lines -> accumulator layout
          if (tls) win.f32_of_lines(res[gb][ii][jp][0], res[gb][ii][jp][1]);
          if constexpr (EPI == EPI_RESID_ROWS || LS) {
            // The row's scale (1 without a table) times the dropout scale (1 when dropout is off: a table of ones gives the plain
            // launch's bits); a dropped row (scale 0) stores the residual itself, whatever the accumulator holds.  RESID_LS: one
            // more rounding for the product with the column's gamma, so a gamma of ones gives the bits of the rows / plain
            // launch; the bf16 image of the branch carries the dropout mask and scale only.
            const float rs = rsc[gb][ii];
            const float cs = p.drop_on ? rs * p.dk.scale : rs;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              bool keep[4] = {true, true, true, true};
              if (p.drop_on) drop_keep4(p.dk, drop_words_a0(p.dk, a0row + (unsigned)i * a0rowstep + a0col[jp][h]), keep);
              float u[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float kv = keep[r] ? v[h][r] : 0.f;
                float sc = cs;
                if constexpr (LS) {
                  u[r] = p.drop_on ? kv * p.dk.scale : kv;
                  sc = cs * gam4[jp][h][r];
                }
                const float t = fmaf(kv, sc, res[gb][ii][jp][h][r]);
                v[h][r] = rs == 0.f ? res[gb][ii][jp][h][r] : t;
              }
              if constexpr (LS) out_a[jp][h] = u32x2{pack_bf2(u[0], u[1]), pack_bf2(u[2], u[3])};
            }
          } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              if (p.drop_on) {
                bool keep[4];
                drop_keep4(p.dk, drop_words_a0(p.dk, a0row + (unsigned)i * a0rowstep + a0col[jp][h]), keep);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[h][r] = fmaf(keep[r] ? v[h][r] : 0.f, p.dk.scale, res[gb][ii][jp][h][r]);
              } else {
                v[h] += res[gb][ii][jp][h];
              }
            }
          }
          store_f32_pair(rsOut0, i, jp, v[0], v[1], nn[jp]);
        } else {   // VITSSL_EPI_EMBED (one launch per step: plain addressing)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (!(okm && okn[jp][h])) continue;
            const long long img = m / p.embed.tokens;
            const int rin = (int)(m - img * p.embed.tokens);
            if (p.embed.mask && p.embed.mask[m]) v[h] = *(const f32x4*)(p.embed.mask_token + nn[jp][h]);
            v[h] += *(const f32x4*)(p.embed.pos + (long long)(p.embed.tok_offset + rin) * p.N + nn[jp][h]);
            const long long orow = img * p.embed.out_tokens + p.embed.tok_offset + rin;
            *(f32x4*)((float*)p.out0 + orow * p.N + nn[jp][h]) = v[h];
          }
        }
        if (CS && p.colsum) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
            if (okm && okn[jp][h]) {
#pragma unroll
              for (int r = 0; r < 4; ++r) csum[2 * jp + h][r] += v[h][r];
            }
        }
      }
      // the row's 128 bytes of every bf16 image leave in back-to-back instructions
      if constexpr (E.windowed && E.out0_esz == 2) {
        // fp8 path: the bf16 image of a dGELU output is optional once its e4m3 image is written (launch-uniform)
        // g' (out0 of the GELU epilogue) is read again only in backward: its stores are non-temporal (aux 2) so that `a`, which
        // FC2 reads next, keeps its lines (in-step A/B: -0.25 ms per ViT-B step; sc1 = 16 was slower)
        if (!(Q8 && E.q8_of == 0) || p.out0) store_bf16_row(rsOut0, i, out_a, IC<EPI == VITSSL_EPI_GELU ? 2 : 0>{});
      }
      if constexpr (E.out1 == OUT1_REQUIRED) {
        if (!(Q8 && E.q8_of == 1) || p.out1) store_bf16_row(rsOut1, i, out_b, IC<0>{});   // same for the GELU output
      }
      if constexpr (E.out1 == OUT1_OPTIONAL) {
        if (p.out1) store_bf16_row(rsOut1, i, out_a, IC<2>{});          // read again only in backward: non-temporal, like g'
      }
      if constexpr (Q8EPI) {
        if (q8) store_fp8_row(rsOut2, i, out_q);
      }
    }
  }

  if (CS && p.colsum) {
    f32x4 red[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = csum[j][r];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        s += __shfl_xor(s, 8, 64);
        red[j][r] = s;
      }
    }
    if (tls) {
      // One store instruction per wave and tile, 64 lanes on 256 contiguous bytes of the wave's slot row, instead of sixteen
      // with four active lanes each: the 64 column sums of the wave pass through its LDS window (column 16 j + 4 g + r of lane
      // group g -> float slot of that column).
      if ((lane & 15) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4*)(xs + (16 * j + 4 * g4) * 4) = red[j];
      }
      asm volatile("" ::: "memory");                  // (the wave's LDS operations execute in order; this keeps hipcc from reordering them)
      const float v = *(const volatile float*)(xs + lane * 4);
      const int n = n0 + wn * 64 + lane;
      if (n < p.N) p.colsum[(m0 / CFG::WROWS + wm) * p.N + n] = v;      // the wave's slot row (launch_cfg sums them)
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4) + r;
          if ((lane & 15) == 0 && n < p.N) p.colsum[(m0 / CFG::WROWS + wm) * p.N + n] = red[j][r];
        }
    }
  }
  if constexpr (Q8EPI) {
    if (p.qamax) {          // one atomic per wave and tile at most; skipped when the slot already holds a larger value
      qmax = wave_max(qmax);
      unsigned* slot = (unsigned*)p.qamax;
      if (lane == 0 && __float_as_uint(qmax) > __builtin_nontemporal_load(slot)) atomicMax(slot, __float_as_uint(qmax));
    }
  }
}

}  // namespace
