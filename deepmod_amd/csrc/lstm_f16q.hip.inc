// lstm_f16q.hip.inc — the split-f16 step-major BiLSTM window classifier on 16x16x32 MFMAs (included by deepmod_hip.hip after
// lstm_f16s.hip.inc, whose design it keeps: reference graph /root/reference/bin/DeepMod_scripts/myMultiBiRNN.py:38-61; every fp32 product
// a*b = a_hi*b_hi + a_lo*b_hi + a_hi*b_lo on the 16-bit matrix cores with fp32 accumulation; step-major, the state of all three layers on
// the chip, weights streamed L2 -> LDS by LDS-DMA, one wave per SIMD owning 32 windows).
//
// Why a second shape (profiles/r04/ablate_mfma16.txt): the path runs at the part's power limit, and v_mfma_f32_32x32x16_f16 reads and writes
// 16 accumulator registers per 16,384 MACs where v_mfma_f32_16x16x32_f16 moves 4 per 8,192 - half the accumulator traffic per FLOP.  A
// timing-only build of lstm_f16s with every 32x32x16 issued as two 16x16x32 ran 5.8 % faster at equal MACs with the clock at 2.3 instead of
// 2.0 GHz.  This kernel is that change made real:
//
//  * a super-tile = 8 units x 4 gates x 32 windows as before, but computed as FOUR 16x16 tiles: row half A (units 8S..8S+3) / B (8S+4..8S+7)
//    x window half 0 (windows 0..15 of the wave) / 1 (16..31).  Lane l = (n = l % 16, g = l / 16) holds, per 16x16 tile, the four gates
//    i, j, f, o of unit 4 * tile + g for window n: still one LSTM cell per lane and tile, four cells per lane and super-tile, lane-local.
//  * K runs in k32-steps.  The B operand of a 16x16x32 MFMA holds k = 8 g + j (j = 0..7) for window n: register r of a k32-step carries slots
//    (2r, 2r+1) = the cells (row half A, row half B) of super-tile 4t + r - exactly the (hi, lo) f16 pairs the cell update of that super-tile
//    packs, so the new h again leaves the cell update in the registers the next operand wants (one register set per window half).
//    k32-steps of a stage: own 0..2 (units 0..95) | input 0..2 (layers 1, 2) | mixed.  The mixed step carries what is left - own units 96..99,
//    the bias row, input units 96..99 (layer 0: the seven features) - with its THREE products laid side by side along K (round 5): per lane
//    group g the slots (own_hi, own_hi, own_lo, in_hi, in_hi, in_lo, 1, 1) meet the weight slots (w_hi, w_lo, w_hi, v_hi, v_lo, v_hi, b_hi, b_lo)
//    of own unit 96 + g / input unit 96 + g (layer 0: feature g) / the bias (g = 0) in ONE MFMA per 16x16 tile; layer 0 has a second one for
//    feature 4 + g (g = 3: the event length beyond the f16 range, rescaled), which has room for the FOURTH product x_lo w_lo of those features:
//    an event length of 10^4 samples makes products of 10^3, and the term the three-product split drops (2^-22 relative) is then 4x fp32's own
//    round-off - measured 2.3e-5 on the probabilities of reads with stalled events, 1e-6 with the slot filled.  K issued = (192 + 192) x 3 products + 32 for 603 slot-products
//    (layer 0: 192 x 3 + 64 for 324), N = 100 exactly (super-tile 12 has no row half B: not loaded, not multiplied): 25,600 MFMAs per 32 windows
//    and direction = 2.94 issued per algorithmic unit (round 4, the mixed step as three products of a 9-slot operand: 28,350 = 3.25).
//  * weights: [dir][layer][super-tile][own 0..2 | input 0..2 : [row half][hi|lo][lane][8 x f16] | mixed : [row half][lane][8 x f16]] = 26 KB per
//    super-tile (16 KB layer 0: own 0..2, then the two mixed records); the ring has 4 x 26 KB slots in the three-product mode, where the super-tiles
//    of a stage run in groups of one or two between barriers (ring_slots below; profiles/edges), and 2 x 26 KB in the int8 mode.
//  * inside an ordinary k32-step the twelve MFMAs run in the snake order: each changes one operand against its predecessor, each accumulator
//    still takes its three products in the order 0, 1, 2 (profiles/r05/ablate_sched.txt; the only order since profiles/edges).
//  * everything else as in lstm_f16s.hip.inc: tile-major, the cell update of the super-tile before cut into chunks between the MFMAs, c of
//    layer 0 in LDS and of layers 1, 2 in registers, the zero-state k32-steps of step 0 skipped, partial logits per direction.
#ifndef DM16Q_TRANS_COST
#define DM16Q_TRANS_COST 2      // issue cost of a transcendental in units of a plain VALU instruction (the cell update is cut into chunks of equal cost)
#endif
namespace lstm16q {

using lstmc::floatx2;
using lstmc::floatx4;
using lstmc::halfx2;
using lstmc::halfx8;
using lstmc::uintx4;
using lstmc::Params;
using lstmc::ex2;
using lstmc::rcp;
using lstmc::min60;      // a compiler-issued v_med3_f32: an inline-asm v_min_f32 here read MFMA results two wait states after the 4-pass MFMA (tools/q_debug.py)
using lstmc::split_pack;
using lstmc::static_for;
using lstmc::as_h8;

constexpr int HID = 100, NFEAT = 7, WIN = 21, LIVE = 11;
constexpr int NTILE = 13;                        // super-tiles of 8 units
constexpr int WAVES = 4, THREADS = 64 * WAVES, TILE_M = 32 * WAVES;
constexpr int KS_L0 = 4, KS_L12 = 7;             // k32-steps per stage
constexpr int REC_BYTES = 4096;                  // one (super-tile, k32-step) record: row half A: hi 1 KB | lo 1 KB, row half B: hi | lo
constexpr int MIX_BYTES = 2048;                  // one mixed record (its three products side by side along K): row half A 1 KB | row half B 1 KB; layer 0 has two
constexpr int TILE_BYTES_L0 = (KS_L0 - 1) * REC_BYTES + 2 * MIX_BYTES, TILE_BYTES_L12 = (KS_L12 - 1) * REC_BYTES + MIX_BYTES;      // 16 KB, 26 KB
constexpr int SLOT_BYTES = TILE_BYTES_L12;
// Ring depth per mode.  The int8 mode (MM 1) parks layer 1's cell state in LDS (its registers hold the int32 accumulators) and keeps the two-slot ring:
// super-tile T + 1 lands in the other slot under super-tile T, one DMA wait and one barrier per super-tile.  The three-product mode (MM 0) has those
// 52 KB for two more slots and runs TWO super-tiles ahead: super-tile g of the stream (13 per stage, stage after stage) sits in slot g % 4 and issues,
// before its first MFMA, the DMA of super-tile g + 2 into slot (g + 2) % 4.  The 13 super-tiles of a stage form the groups {0}, {1, 2}, {3, 4}, ...,
// {11, 12}, and only the LAST super-tile of a group (T even) ends with s_waitcnt vmcnt(0) and s_barrier - 7 per stage instead of 13
// (profiles/edges/README.md).
//  * the grouping is a compile-time property of T: every barrier is unconditional, every wave of a workgroup executes the same 7 per stage and
//    231 per work item whatever its data, so no wave can wait at a barrier another one never reaches; nothing polls or waits on memory.
//  * the slot written under super-tile g was last read by super-tile g - 2, which lies in an EARLIER group for every T (T odd: the barrier after
//    T - 1; T even: the one after T - 2; T = 0, 1: the one after super-tile 12 of the stage before), so every wave has left it; it is neither g's
//    own slot nor that of g's partner in the group (g - 1 or g + 1).
//  * super-tile g + 2 lies in a LATER group than g (T odd: behind the barrier after T + 1; T even, and T = 11, 12 into the next stage: behind the
//    one after T or 12), and a wave reaches that barrier only after waiting for all its own pieces: what a group reads is complete.
// A stage has an odd number of super-tiles, so pairs that ran on across stages would make the position of the barrier a run-time property of the step
// (or a second copy of the step's code: the kernel's 3,550 static MFMAs are pinned); one single per stage costs one barrier in 39 super-tiles more.
__host__ __device__ constexpr int ring_slots(int mm) {
#ifdef DM16Q_ABL_PAIRBAR
    return 2;
#else
    return mm == 0 ? 4 : 2;
#endif
}
constexpr int C2_WAVE_BYTES = NTILE * 1024;      // cell state of layer 0 for one wave: [super-tile][lane][4 fp32]
constexpr int C2_LAYER_BYTES = WAVES * C2_WAVE_BYTES;
constexpr size_t LDS_BYTES = size_t(ring_slots(0)) * SLOT_BYTES + C2_LAYER_BYTES;          // 106,496 + 53,248 = 159,744 B
constexpr size_t LDS_BYTES_I8 = size_t(ring_slots(1)) * SLOT_BYTES + 2 * C2_LAYER_BYTES;   // 53,248 + 106,496 = 159,744 B as well
constexpr size_t WEIGHT_BYTES_DIR = size_t(NTILE) * (TILE_BYTES_L0 + 2 * TILE_BYTES_L12);
constexpr size_t WEIGHT_BYTES = 2 * WEIGHT_BYTES_DIR;                              // 1,810,432 B

// Four LSTM cells of one lane (cell q = 2 * window half + row half), cut into single instructions so that they can be issued between the
// MFMAs of the next super-tile; the formulas of lstm16s::CellPipe (pre-activations pre-scaled by the packer: i, f, o columns
// x -log2(e), j column x 2 log2(e); cell state carried as c2 = 2 log2(e) c):
//     c2' = c2 / (1 + 2^af) + 2 log2(e) (2^aj - 1) / ((1 + 2^ai)(1 + 2^aj));   h = (2^c2' - 1) / ((1 + 2^c2')(1 + 2^ao))
// in 19 instead of 22 instructions per cell (round 5: 5 v_exp, 3 v_rcp, 11 plain): both products of two (1 + 2^x) terms are one fma
// (a b + b with b = 1 + 2^y) instead of add + mul, and c2' is not clamped before its exponential - |c| < 11 after 11 steps from the zero state.
// The launch runs at the board's power limit, where an instruction not issued is time: -2.8 % (profiles/r05/ablate_cell19.txt).
// The op list of a super-tile depends on two compile-time properties (lstm16s::CellPipe has the same two; DM_PREC_F16X3 is PRE = FMT = 0):
//   PRE 1: the super-tile's cross terms were accumulated as int32 (DM_PREC_F16I8 on this shape, round 5): 16 v_cvt_f32_i32 + 8 v_pk_fma_f32 fold
//          them into the fp32 pre-activations first (g += S[gate] * n)
//   FMT    what the new h is packed into: 0 (hi, lo) f16 pairs | 1 hi f16 pairs + int8 pairs (lo8 = rint(lo 127 2^12), hi8 = rint(h 127): bytes
//          (lo8, hi8) per unit, the B operand of v_mfma_i32_16x16x64_i8) | 2 both (layer 2: its last stage feeds the head in f16)
// Micro-steps m: 0 fold | 1..9 gates .. h and the hi packs | 10 hi8 | 11 lo = h - hi | 12 lo f16 packs | 13 lo8 and the int8 packs.
using lstmc::intx4;
using lstmc::I8_MAGIC;
using lstmc::I8_HI_SCALE;
using lstmc::I8_LO_SCALE;
struct CellPipe {
    float ef[4], ei[4], ej[4], eo[4], t0[4], t1[4];
    unsigned hi01, hi23, lo01, lo23, i01, i23;
    floatx2 fold[2];
    floatx2 kmagic, khi, klo;      // int8 formats: (MAGIC, MAGIC), (127, 127), (127 * 2^12, 127 * 2^12) in registers (a packed fma takes one scalar pair at most)
    static constexpr int NM = 14;
    template <int PRE, int FMT>
    __device__ static constexpr int nops(int M) {
        constexpr int n[9] = {12, 12, 12, 12, 8, 4, 4, 8, 6};
        if (M == 0) return PRE ? 16 : 0;
        if (M <= 9) return n[M - 1];
        if (M == 10) return FMT >= 1 ? 2 : 0;
        if (M == 11) return 4;
#if defined(DM16Q_LOPACK)      // experiment (round 6, VERDICT r05 item 3a): 1 = the lo halves packed by v_fma_mixlo / mixhi_f16 straight from h - hi (micro-step 11 writes the pairs, 12 disappears
                               // for FMT 0); 2 = timing only: micro-step 12 dropped, the lo operand IS the hi operand (what the two conversions per super-tile cost)
        if (M == 12) return FMT == 2 ? 2 : 0;
#else
        if (M == 12) return FMT != 1 ? 2 : 0;
#endif
        return FMT >= 1 ? 8 : 0;
    }
    // instruction J of micro-step M: level-major over the four cells, so consecutive instructions are independent.
    // only_a: super-tile 12 has row half A only (units 96..99): cells 1 and 3 (row half B: units 100..103 do not exist) are not issued
    // (super-tile 12 always packs FMT 0: its units ride the mixed k32-step, which stays in f16)
    template <int M, int J, int FMT = 0>
    __device__ __forceinline__ void op(floatx4 (&g)[4], const intx4 (&gi)[4], const floatx2 (&S)[2], float* c2, const bool only_a) {
        constexpr float K2 = 2.0f * 1.4426950408889634f;
        constexpr int q = J & 3, lv = J >> 2;
#define DM_PIN(X) asm volatile("" : "+v"(X))
        if constexpr (M == 0) {             // fold of the int32 cross terms of cell k / 2, gates (2 (k % 2), 2 (k % 2) + 1): two conversions, then one packed fma
            constexpr int k = J >> 1, c = k >> 1, pr = k & 1;
            if (only_a && (c & 1)) return;
            if constexpr ((J & 1) == 0) {
                fold[pr] = floatx2{(float)gi[c][2 * pr], (float)gi[c][2 * pr + 1]};
            } else {
                const floatx2 gp = __builtin_elementwise_fma(fold[pr], S[pr], floatx2{g[c][2 * pr], g[c][2 * pr + 1]});
                g[c][2 * pr] = gp[0];
                g[c][2 * pr + 1] = gp[1];
            }
            return;
        }
        if (only_a && (((M <= 8 || M == 11) && (q & 1)) || (M == 9 && lv == 0 && (q & 1)))) return;
        if constexpr (M == 1) {
            if constexpr (lv == 0) { t0[q] = min60(g[q][1]); DM_PIN(t0[q]); }
            else if constexpr (lv == 1) { ef[q] = ex2(g[q][2]); DM_PIN(ef[q]); }
            else { ei[q] = ex2(g[q][0]); DM_PIN(ei[q]); }
        } else if constexpr (M == 2) {
            if constexpr (lv == 0) { ej[q] = ex2(t0[q]); DM_PIN(ej[q]); }
            else if constexpr (lv == 1) { eo[q] = ex2(g[q][3]); DM_PIN(eo[q]); }
            else { ef[q] = 1.0f + ef[q]; DM_PIN(ef[q]); }
        } else if constexpr (M == 3) {       // ef <- sigma(f) = 1 / (1 + 2^af); t0 <- 2 log2(e) (2^aj - 1)
            if constexpr (lv == 0) { ef[q] = rcp(ef[q]); DM_PIN(ef[q]); }
            else if constexpr (lv == 1) { t1[q] = 1.0f + ej[q]; DM_PIN(t1[q]); }
            else { t0[q] = fmaf(ej[q], K2, -K2); DM_PIN(t0[q]); }
        } else if constexpr (M == 4) {
            if constexpr (lv == 0) { ei[q] = fmaf(ei[q], t1[q], t1[q]); DM_PIN(ei[q]); }      // (1 + 2^ai)(1 + 2^aj) in one fma
            else if constexpr (lv == 1) { eo[q] = 1.0f + eo[q]; DM_PIN(eo[q]); }
            else { ei[q] = rcp(ei[q]); DM_PIN(ei[q]); }
        } else if constexpr (M == 5) {
            if constexpr (lv == 0) { t0[q] = t0[q] * ei[q]; DM_PIN(t0[q]); }
            else { c2[q] = fmaf(c2[q], ef[q], t0[q]); DM_PIN(c2[q]); }
        } else if constexpr (M == 6) {
            { t0[q] = ex2(c2[q]); DM_PIN(t0[q]); }      // no clamp: |c| < 11 after 11 steps from the zero state (|i tanh j| < 1, f < 1), so c2 = 2 log2(e) c < 32
        } else if constexpr (M == 7) {
            { t1[q] = t0[q] - 1.0f; DM_PIN(t1[q]); }
        } else if constexpr (M == 8) {
            if constexpr (lv == 0) { t0[q] = fmaf(t0[q], eo[q], eo[q]); DM_PIN(t0[q]); }      // (1 + 2^c2')(1 + 2^ao) in one fma
            else { t0[q] = rcp(t0[q]); DM_PIN(t0[q]); }
        } else if constexpr (M == 9) {       // t1 <- h; then the hi halves, packed: (cell 0, cell 1) = window half 0, (cell 2, cell 3) = window half 1
            if constexpr (lv == 0) { t1[q] = t1[q] * t0[q]; DM_PIN(t1[q]); }
            else if constexpr (J == 4) { hi01 = __builtin_bit_cast(unsigned, halfx2{(_Float16)t1[0], (_Float16)t1[1]}); DM_PIN(hi01); }
            else { hi23 = __builtin_bit_cast(unsigned, halfx2{(_Float16)t1[2], (_Float16)t1[3]}); DM_PIN(hi23); }
        } else if constexpr (M == 10) {      // hi8: h * 127 rounded to an integer in the low byte (ef is free by now), two cells per instruction
            const floatx2 v = __builtin_elementwise_fma(floatx2{t1[2 * J], t1[2 * J + 1]}, khi, kmagic);
            ef[2 * J] = v[0];
            ef[2 * J + 1] = v[1];
        } else if constexpr (M == 11) {      // lo = h - (float)hi in one v_fma_mix_f32 (the SAME conversion that was packed: lo is what it left)
#if defined(DM16Q_LOPACK) && DM16Q_LOPACK == 1
            if constexpr (FMT == 0) {        // ... rounded to f16 and written into its half of the pair by the same instruction
                if constexpr (q == 0) asm volatile("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(lo01) : "v"(hi01), "v"(t1[0]));
                else if constexpr (q == 1) asm volatile("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo01) : "v"(hi01), "v"(t1[1]));
                else if constexpr (q == 2) asm volatile("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(lo23) : "v"(hi23), "v"(t1[2]));
                else asm volatile("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo23) : "v"(hi23), "v"(t1[3]));
                return;
            }
#elif defined(DM16Q_LOPACK) && DM16Q_LOPACK == 2
            if constexpr (FMT == 0) {        // timing only: no lo pack at all
                if constexpr (q == 0) lo01 = hi01;
                if constexpr (q == 2) lo23 = hi23;
            }
#endif
            if constexpr ((q & 1) == 0) asm volatile("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(t1[q]) : "v"(q < 2 ? hi01 : hi23));
            else asm volatile("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(t1[q]) : "v"(q < 2 ? hi01 : hi23));
        } else if constexpr (M == 12) {
            if constexpr (J == 0) { lo01 = __builtin_bit_cast(unsigned, halfx2{(_Float16)t1[0], (_Float16)t1[1]}); DM_PIN(lo01); }
            else { lo23 = __builtin_bit_cast(unsigned, halfx2{(_Float16)t1[2], (_Float16)t1[3]}); DM_PIN(lo23); }
        } else {                             // M == 13: lo8 (ei is free), then bytes (lo8, hi8) of two cells per register
            if constexpr (J < 2) {
                const floatx2 v = __builtin_elementwise_fma(floatx2{t1[2 * J], t1[2 * J + 1]}, klo, kmagic);
                ei[2 * J] = v[0];
                ei[2 * J + 1] = v[1];
            } else {
                // v_perm_b32 D, S0, S1, sel: selector byte 0..3 = byte of S1, 4..7 = byte of S0, 0x0C = 0x00
                constexpr int c = J < 5 ? 0 : 2;                // first cell of the pair
                constexpr int k = J < 5 ? J - 2 : J - 5;
                if constexpr (k == 0) { t0[c] = __builtin_bit_cast(float, __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, ef[c]), __builtin_bit_cast(unsigned, ei[c]), 0x0C0C0400u)); DM_PIN(t0[c]); }
                else if constexpr (k == 1) { t0[c + 1] = __builtin_bit_cast(float, __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, ef[c + 1]), __builtin_bit_cast(unsigned, ei[c + 1]), 0x0C0C0400u)); DM_PIN(t0[c + 1]); }
                else {
                    const unsigned r = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, t0[c + 1]), __builtin_bit_cast(unsigned, t0[c]), 0x05040100u);
                    if constexpr (c == 0) { i01 = r; DM_PIN(i01); } else { i23 = r; DM_PIN(i23); }
                }
            }
        }
#undef DM_PIN
    }
    template <int PRE, int FMT>
    __device__ static constexpr int nops_before(int M) {
        int n = 0;
        for (int m = 0; m < M; ++m) n += nops<PRE, FMT>(m);
        return n;
    }
    template <int PRE, int FMT>
    __device__ static constexpr int nops_all() { return nops_before<PRE, FMT>(NM); }
    template <int PRE, int FMT>
    __device__ static constexpr int op_m(int k) {
        int m = 0;
        while (k >= nops<PRE, FMT>(m)) k -= nops<PRE, FMT>(m++);
        return m;
    }
    template <int PRE, int FMT>
    __device__ static constexpr int op_j(int k) { return k - nops_before<PRE, FMT>(op_m<PRE, FMT>(k)); }
    // issue cost: a transcendental costs two plain VALU issues, the conversion pair of the fold two
    template <int PRE, int FMT>
    __device__ static constexpr int op_cost(int k) {
        const int m = op_m<PRE, FMT>(k), lv = op_j<PRE, FMT>(k) >> 2;
        if (m == 0) return (op_j<PRE, FMT>(k) & 1) ? 1 : 2;
        if (m >= 10) return 1;
        const bool trans = (m == 1 && lv >= 1) || (m == 2 && lv <= 1) || (m == 3 && lv == 0) || (m == 4 && lv == 2) || (m == 6) || (m == 8 && lv == 1);
        return trans ? DM16Q_TRANS_COST : 1;
    }
    template <int PRE, int FMT>
    __device__ static constexpr int cost_before(int k) {
        int c = 0;
        for (int i = 0; i < k; ++i) c += op_cost<PRE, FMT>(i);
        return c;
    }
    template <int PRE, int FMT>
    __device__ static constexpr int chunk_lo(int c, int nch) {      // first op of chunk c of nch (chunks of equal issue cost)
        const int W = cost_before<PRE, FMT>(nops_all<PRE, FMT>());
        int k = 0;
        while (k < nops_all<PRE, FMT>() && cost_before<PRE, FMT>(k) * nch < c * W) ++k;
        return k;
    }
    template <int C, int NCH, int PRE, int FMT>
    __device__ __forceinline__ void chunk(floatx4 (&g)[4], const intx4 (&gi)[4], const floatx2 (&S)[2], float* c2, const bool only_a) {
#ifdef DM16Q_ABL_NOCELL
        return;
#endif
        if constexpr (C < NCH) {
            constexpr int LO = chunk_lo<PRE, FMT>(C, NCH), HI = chunk_lo<PRE, FMT>(C + 1, NCH);
            static_for<HI - LO>([&](auto kc) {
                constexpr int k = LO + decltype(kc)::value;
                this->template op<op_m<PRE, FMT>(k), op_j<PRE, FMT>(k), FMT>(g, gi, S, c2, only_a);
            });
        }
    }
    template <int PRE, int FMT>
    __device__ __forceinline__ void all(floatx4 (&g)[4], const intx4 (&gi)[4], const floatx2 (&S)[2], float* c2, const bool only_a) { chunk<0, 1, PRE, FMT>(g, gi, S, c2, only_a); }
};

// LDS-DMA of one weight tile into a ring slot: the 4 waves take contiguous runs of 1 KB pieces (26 KB of layers 1, 2: 7, 7, 6, 6).
template <int TILE_BYTES>
__device__ __forceinline__ void stage_tile(const unsigned char* gtile /*uniform*/, unsigned lds_slot /*uniform*/, int wave_s, unsigned lane16) {
#ifdef DM16Q_ABL_NODMA
    return;
#endif
    constexpr int NKB = TILE_BYTES / 1024, BASE = NKB / WAVES, REM = NKB % WAVES;
    static_assert(TILE_BYTES % 1024 == 0 && BASE >= 1 && BASE + (REM ? 1 : 0) <= 7, "pieces per wave");
    const int kb0 = wave_s * BASE + (wave_s < REM ? wave_s : REM);
    const unsigned char* g = gtile + kb0 * 1024 + 4096;
    const unsigned l = lds_slot + unsigned(kb0) * 1024u + 4096u;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0" : "=&s"(keep) : "s"(l) : "memory");
#define DM_PIECE(J) if constexpr ((J) < BASE) asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" :: "v"(lane16), "s"(g), "i"((J) * 1024 - 4096) : "memory");
    DM_PIECE(0) DM_PIECE(1) DM_PIECE(2) DM_PIECE(3) DM_PIECE(4) DM_PIECE(5) DM_PIECE(6)
#undef DM_PIECE
    if constexpr (REM > 0) {      // the first REM waves take one piece more; the skip stays inside the asm (a compiler-visible branch would cut the stage into scheduling regions)
        asm volatile("s_cmp_lt_i32 %3, %4\n\ts_cbranch_scc0 .Ldm16q_skip_%=\n\tglobal_load_lds_dwordx4 %0, %1 offset:%2\n.Ldm16q_skip_%=:"
                     :: "v"(lane16), "s"(g), "i"(BASE * 1024 - 4096), "s"(wave_s), "i"(REM) : "memory", "scc");
    }
    asm volatile("s_mov_b32 m0, %0" :: "s"(keep) : "memory");
}

struct AQuad {
    halfx8 hiA, loA, hiB, loB;
};
// A fragments of one k32-step at byte offset OFF of the ring slot.  An ordinary record: hiA, loA (, hiB, loB); MIXED = 1: the one record of
// layers 1, 2 (row half A -> hiA, row half B -> hiB); MIXED = 2: layer 0's two (first -> hiA, hiB; second -> loA, loB)
template <int OFF, bool WITH_B, int MIXED>
__device__ __forceinline__ void load_a(AQuad& a, const unsigned addr) {
    if constexpr (MIXED == 0) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.hiA) : "v"(addr), "i"(OFF));
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.loA) : "v"(addr), "i"(OFF + 1024));
        if constexpr (WITH_B) {
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.hiB) : "v"(addr), "i"(OFF + 2048));
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.loB) : "v"(addr), "i"(OFF + 3072));
        }
    } else {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.hiA) : "v"(addr), "i"(OFF));
        if constexpr (WITH_B) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.hiB) : "v"(addr), "i"(OFF + 1024));
        if constexpr (MIXED == 2) {
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.loA) : "v"(addr), "i"(OFF + MIX_BYTES));
            if constexpr (WITH_B) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a.loB) : "v"(addr), "i"(OFF + MIX_BYTES + 1024));
        }
    }
}
__host__ __device__ constexpr int a_reads(bool with_b, int mixed) { return (mixed == 1 ? 1 : 2) * (with_b ? 2 : 1); }
template <int N>
__device__ __forceinline__ void wait_a(AQuad& a) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a.hiA), "+v"(a.loA), "+v"(a.hiB), "+v"(a.loB) : "i"(N));
}

#define DM16Q_STR2(X) #X
#define DM16Q_STR(X) DM16Q_STR2(X)
#if defined(DM16Q_NOPN)
#define DM16Q_AFTER_MFMA "s_nop " DM16Q_STR(DM16Q_NOPN)
#elif defined(DM16Q_DEBUG_NOP)
#define DM16Q_AFTER_MFMA "s_nop 15\n\ts_nop 15"
#else
#define DM16Q_AFTER_MFMA ""
#endif
#ifndef DM16Q_PRE
#define DM16Q_PRE 2      // cell-update chunks issued before the first MFMA of a super-tile
#endif

// FIRST = the stages of step 0: the hidden state is exactly zero, the own k32-steps 0..2 are skipped (bit-identical: their products are +0)
template <int LAYER, bool FIRST>
struct StageKind {
    static constexpr bool L0 = LAYER == 0;
    static constexpr int KS_FULL = L0 ? KS_L0 : KS_L12;
    static constexpr int KS = FIRST ? KS_FULL - 3 : KS_FULL;             // k32-steps in processing order: [own 0..2 | input 0..2 | mixed]
    static constexpr int TILE_BYTES = L0 ? TILE_BYTES_L0 : TILE_BYTES_L12;
    static constexpr int DMA_OFF = FIRST ? 3 * REC_BYTES : 0;
    static constexpr int DMA_BYTES = TILE_BYTES - DMA_OFF;
    static constexpr int rec_off(int i) { return (FIRST ? 3 + i : i) * REC_BYTES; }       // records lie in processing order, the mixed one last
    static constexpr int mixed(int i) { return i == KS - 1 ? (L0 ? 2 : 1) : 0; }          // 0: an ordinary k32-step, 1 / 2: the mixed step with one / two records
    static constexpr bool is_own(int i) { return !FIRST && i < 3; }
    static constexpr int opnd(int i) { return FIRST ? i : (i < 3 ? i : i - 3); }          // k32-step 0..2 of the own / input operand
};

constexpr int quad(int t, int hh, int part) { return (t * 2 + hh) * 2 + part; }      // B-operand quad of k32-step t (0..2), window half, hi | lo

struct WaveState {
    uintx4 own[3][12];        // hidden state of the three layers, units 0..95, as B-operand quads
    unsigned m12[3][2][2];    // unit 96 + g of the three layers as the mixed k32-step wants it: [layer][window half][(hi, hi) | (hi, lo)]
    uintx4 nxt[12];           // the h the running stage produces (units 0..95)
    float c2reg[NTILE][4];    // cell state of layer 2
    float c1reg[NTILE][4];    // cell state of layer 1 (layer 0: LDS; the int8 mode: LDS as well)
    floatx4 acc[3][4];        // super-tile T accumulates in acc[T == 12 ? 2 : T & 1][2 * window half + row half]
    intx4 acci[3][4];         // int8 mode: the cross terms of the same super-tile (int32), folded into acc by the cell update
    floatx2 i8s[3][2];        // int8 mode: fold scales of this direction, [layer][gates (i, j) | (f, o)]
    CellPipe cp;
    float xf[2][2];           // this lane's features of the NEXT layer-0 stage: [window half][feature g | feature 4 + g]
    int slot;
};

// cell-state row of (layer, super-tile) of this lane: registers for layer 2 and (three-product mode) layer 1, LDS otherwise
template <int LAYER, int MM>
__device__ __forceinline__ void c2_load(WaveState& w, const unsigned c2lds, const int tile, float (&row)[4]) {
    if constexpr (LAYER == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) row[q] = w.c2reg[tile][q];
    } else if constexpr (LAYER == 1 && MM == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) row[q] = w.c1reg[tile][q];
    } else {
        floatx4 v;
        // no wait here: LDS returns in order, the next wait for A fragments covers it (it leaves only reads issued after this one outstanding)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(c2lds), "i"(LAYER * C2_LAYER_BYTES));
#pragma unroll
        for (int q = 0; q < 4; ++q) row[q] = v[q];
    }
}
template <int LAYER, int MM>
__device__ __forceinline__ void c2_store(WaveState& w, const unsigned c2lds, const int tile, const float (&row)[4]) {
    if constexpr (LAYER == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) w.c2reg[tile][q] = row[q];
    } else if constexpr (LAYER == 1 && MM == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) w.c1reg[tile][q] = row[q];
    } else {
        asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(c2lds), "v"(floatx4{row[0], row[1], row[2], row[3]}), "i"(LAYER * C2_LAYER_BYTES) : "memory");
    }
}

// (low half, high half) -> one register; the halves of the mixed k32-step's B operand
__device__ __forceinline__ unsigned lo_lo(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }      // (a.low, b.low)
__device__ __forceinline__ unsigned hi_lo(unsigned a, unsigned b) { return __builtin_amdgcn_alignbit(b, a, 16); }          // (a.high, b.low)

// One stage = one layer at one step: 13 super-tiles.  PREV = the layer of the stage before (whose super-tile 12 still owes its cells).
// MM 0: three f16 products (DM_PREC_F16X3).  MM 1 (DM_PREC_F16I8 on this shape, round 5): the ordinary k32-steps run a_hi w_hi in f16 and BOTH
// cross terms as ONE v_mfma_i32_16x16x64_i8 per 16x16 tile - B bytes (lo8, hi8) per unit against A bytes (w_hi8, w_lo8), an int32 accumulator
// per tile, folded into the fp32 pre-activations by the cell update; the mixed k32-step (own / input units 96..99, bias, features) keeps its three
// f16 products in one MFMA, so super-tile 12 always packs (hi, lo) f16.  8 + 8 instead of 12 + 12 MFMAs per two k32-steps: 17,800 per 32 windows
// and direction instead of 25,600.  Same reduced-precision contract as lstm16s::bilstm_f16s_kernel<1> (include/deepmod_hip.h).
template <int LAYER, bool FIRST, int MM>
__device__ __forceinline__ void run_stage(const Params& p, WaveState& w, const unsigned lds_base, const unsigned c2_wave, const unsigned char* wdir, const int dir, const int s,
                                          const float* xwin0, const float* xwin1, const int wave_s, const unsigned lane16, const int grp, const unsigned one2) {
    using K = StageKind<LAYER, FIRST>;
    constexpr bool L0 = K::L0;
    constexpr int KS = K::KS;
    constexpr int PREV = (LAYER + 2) % 3;
    constexpr int I8 = (MM == 1 && !(L0 && FIRST)) ? 1 : 0;          // does this stage issue int8 MFMAs (layer 0 at step 0 is its mixed k32-step alone)
    constexpr int PRE = I8;                                          // ... then its super-tiles are folded
    constexpr int PPRE = (MM == 1 && !(PREV == 0 && FIRST)) ? 1 : 0; // super-tile 12 of the stage before (layer 2 at step 0 is an int8 stage; before the first stage: zero counts)
    constexpr int FMT = MM == 0 ? 0 : (LAYER == 2 ? 2 : 1);          // super-tiles 0..11 of this stage; super-tile 12: always 0
    constexpr size_t LAYER_OFF[3] = {0, size_t(NTILE) * TILE_BYTES_L0, size_t(NTILE) * (TILE_BYTES_L0 + TILE_BYTES_L12)};
    uintx4 (&own)[12] = w.own[LAYER];
    const uintx4 (&inp)[12] = w.own[L0 ? 0 : LAYER - 1];
    const floatx2 (&S)[2] = w.i8s[LAYER];
    const floatx2 (&PS)[2] = w.i8s[PREV];
    uintx4 mx[2], mx2[2];                                        // mixed k32-step operand(s) per window half
    unsigned x0p[2] = {0u, 0u}, x1a[2] = {0u, 0u}, x1b[2] = {0u, 0u};
    if constexpr (L0) {
        // this stage's feature row for the mixed k32-step: feature g as (hi, lo), feature 4 + g as (hi, hi) and (lo, lo); the event length (a raw sample count) rides
        // BOTH slots, cut at 2^len_shift: g = 3 carries t = rint(length 2^-len_shift) against the weight row stored x 2^len_shift, g = 2 the rest
        // (|rest| <= 2^(len_shift - 1)) against the row as it is - see lstm_f16s.hip.inc
        bool bad = false;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            float v0 = w.xf[hh][0], v1 = w.xf[hh][1];
            bad |= !(fabsf(v0) <= 65504.0f);
            if (grp < 2) bad |= !(fabsf(v1) <= 65504.0f);
            else {                                                      // the event length = t 2^len_shift + rest (lstm_f16s.hip.inc: same rule)
                const float t = rintf(v1 * p.len_scale);
                bad |= !(fabsf(t) <= 65504.0f);
                v1 = grp == 2 ? v1 - t * p.len_mul : t;
            }
            unsigned xh, xl;
            split_pack(v0, v1, xh, xl);                                 // xh = (hi v0, hi v1), xl = (lo v0, lo v1)
            x0p[hh] = lo_lo(xh, xl);
            x1a[hh] = __builtin_amdgcn_perm(xh, xh, 0x03020302u);       // (hi v1, hi v1)
            x1b[hh] = __builtin_amdgcn_perm(xl, xl, 0x03020302u);       // (lo v1, lo v1): the second one meets w_lo - see below
        }
        if (bad) *p.range_flag = 1;
        if (s + 1 < LIVE) {                                             // next step's feature row, one step ahead
            const int row = dir == 0 ? s + 1 : WIN - 2 - s;
            const int f1 = 4 + grp < NFEAT ? 4 + grp : NFEAT - 1;
            w.xf[0][0] = xwin0[row * NFEAT + grp]; w.xf[0][1] = xwin0[row * NFEAT + f1];
            w.xf[1][0] = xwin1[row * NFEAT + grp]; w.xf[1][1] = xwin1[row * NFEAT + f1];
        }
    }
    const bool last_stage = LAYER == 2 && s == LIVE - 1;
#ifdef DM16Q_AINIT
    AQuad a[2] = {};
#else
    AQuad a[2];                                                         // A fragments, double-buffered over the k32-steps; across the super-tiles of a group: see PF_OUT
#endif
    static_for<NTILE>([&](auto Tc) {
        constexpr int T = decltype(Tc)::value;
        constexpr int P = T == 0 ? NTILE - 1 : T - 1;                   // the super-tile whose cells are updated under this one's MFMAs
        constexpr int accT = T == NTILE - 1 ? 2 : (T & 1), accP = P == NTILE - 1 ? 2 : (P & 1);
        constexpr bool WITH_B = T < NTILE - 1;                          // super-tile 12 has row half A only
        constexpr int NMF = (WITH_B ? 4 : 2) * (I8 ? 2 : 3);            // MFMAs of one ordinary k32-step
        float c2row[4];
        if constexpr (T == 0) c2_load<PREV, MM>(w, c2_wave + unsigned(NTILE - 1) * 1024u, NTILE - 1, c2row);
        else c2_load<LAYER, MM>(w, c2_wave + unsigned(P) * 1024u, P, c2row);
        const unsigned a_addr = lds_base + unsigned(w.slot) * SLOT_BYTES + lane16;
        constexpr int NS = ring_slots(MM);
        constexpr bool EDGE = NS == 2 || (T & 1) == 0;                  // the last super-tile of its group: the DMA wait and the barrier below
        // no barrier between the two super-tiles of a group: the first one (PF_OUT) reads the second one's first A fragments before its own last k32-step,
        // into the buffer that step does not use, and the second one (PF_IN) starts on that buffer (AOFS) instead of reading them behind the last MFMA
        constexpr bool PF_OUT = NS == 4 && (T & 1) == 1, PF_IN = NS == 4 && T >= 2 && (T & 1) == 0;
        constexpr int AOFS = PF_IN ? (KS & 1) : 0;
        if constexpr (!PF_IN) load_a<K::rec_off(0), WITH_B, K::mixed(0)>(a[0], a_addr);
        // ---- super-tile g + AHEAD of the weight stream -> ring slot (g + AHEAD) % NS (see ring_slots); all pieces first (profiles/r05/ablate_dma_spread.txt: later is worse) ----
        constexpr int AHEAD = NS / 2;
        if constexpr (T + AHEAD < NTILE) {
            unsigned toff = unsigned(T + AHEAD) * K::TILE_BYTES;
            asm volatile("" : "+s"(toff));
            stage_tile<K::DMA_BYTES>(wdir + (LAYER_OFF[LAYER] + K::DMA_OFF) + toff, lds_base + unsigned((w.slot + AHEAD) & (NS - 1)) * SLOT_BYTES + K::DMA_OFF, wave_s, lane16);
        } else if (!last_stage) {                                       // (the stream ends with the last stage)
            using KN = StageKind<(LAYER + 1) % 3, FIRST && LAYER < 2>;
            constexpr size_t noff = size_t(T + AHEAD - NTILE) * KN::TILE_BYTES;
            stage_tile<KN::DMA_BYTES>(wdir + (LAYER_OFF[(LAYER + 1) % 3] + KN::DMA_OFF + noff), lds_base + unsigned((w.slot + AHEAD) & (NS - 1)) * SLOT_BYTES + KN::DMA_OFF, wave_s, lane16);
        }
        floatx4 (&d)[4] = w.acc[accT];
        intx4 (&di)[4] = w.acci[accT];
        floatx4 (&g)[4] = w.acc[accP];
        const intx4 (&gi)[4] = w.acci[accP];
        const floatx4 z4 = {0.f, 0.f, 0.f, 0.f};
        const intx4 zi4 = {0, 0, 0, 0};
        constexpr int NCH = DM16Q_PRE + NMF * (KS - 1);
        // the update of super-tile P as chunk C of NCH: super-tile 12 of the stage before under super-tile 0 (its fold as that stage was, its packs f16), else this stage's T - 1
#ifdef DM16Q_NOCHUNK      // debug: the whole cell update of super-tile P as one block before the last k32-step
#define DM_CHUNK(C) do { if constexpr ((C) == NCH - 1) { if constexpr (T == 0) w.cp.template all<PPRE, 0>(g, gi, PS, c2row, true); else w.cp.template all<PRE, FMT>(g, gi, S, c2row, false); } } while (0)
#else
#define DM_CHUNK(C) do { if constexpr (T == 0) w.cp.template chunk<(C), NCH, PPRE, 0>(g, gi, PS, c2row, true); else w.cp.template chunk<(C), NCH, PRE, FMT>(g, gi, S, c2row, false); } while (0)
#endif
        if constexpr (KS > 1) static_for<DM16Q_PRE>([&](auto cc) { DM_CHUNK(decltype(cc)::value); });
        static_for<KS>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int MIXED = K::mixed(i);
            AQuad& ai = a[(i + AOFS) & 1];
            if constexpr (i + 1 < KS) load_a<K::rec_off(i + 1), WITH_B, K::mixed(i + 1)>(a[(i + 1 + AOFS) & 1], a_addr);
            if constexpr (i == KS - 1) {
                // the cells of super-tile P are done: their (hi, lo) pairs become operands, their state goes back
                if constexpr (KS == 1) {                                   // (layer 0 at step 0: one k32-step, nothing to hide under)
                    if constexpr (T == 0) w.cp.template all<PPRE, 0>(g, gi, PS, c2row, true);
                    else w.cp.template all<PRE, FMT>(g, gi, S, c2row, false);
                }
#ifdef DM16Q_ABL_NOCELL
                w.cp.hi01 = w.cp.hi23 = 0x2E662E66u; w.cp.lo01 = w.cp.lo23 = 0x0A660A66u;
#endif
                if constexpr (T == 0) {
                    // super-tile 12 of the stage before: unit 96 + g = cells 0 (window half 0) and 2 (window half 1), in the LOW halves of the packs
                    w.m12[PREV][0][0] = lo_lo(w.cp.hi01, w.cp.hi01); w.m12[PREV][0][1] = lo_lo(w.cp.hi01, w.cp.lo01);
                    w.m12[PREV][1][0] = lo_lo(w.cp.hi23, w.cp.hi23); w.m12[PREV][1][1] = lo_lo(w.cp.hi23, w.cp.lo23);
                    c2_store<PREV, MM>(w, c2_wave + unsigned(NTILE - 1) * 1024u, NTILE - 1, c2row);
                } else {
                    constexpr int pt = P >> 2, pr = P & 3;             // k32-step and register of super-tile P's slots
                    unsigned s01, s23;                                  // the second halves: lo f16 pairs, or int8 pairs (layer 2: f16 from its last stage, for the head)
                    if constexpr (FMT == 0) { s01 = w.cp.lo01; s23 = w.cp.lo23; }
                    else if constexpr (FMT == 1) { s01 = w.cp.i01; s23 = w.cp.i23; }
                    else { s01 = last_stage ? w.cp.lo01 : w.cp.i01; s23 = last_stage ? w.cp.lo23 : w.cp.i23; }
                    w.nxt[quad(pt, 0, 0)][pr] = w.cp.hi01; w.nxt[quad(pt, 0, 1)][pr] = s01;
                    w.nxt[quad(pt, 1, 0)][pr] = w.cp.hi23; w.nxt[quad(pt, 1, 1)][pr] = s23;
                    c2_store<LAYER, MM>(w, c2_wave + unsigned(P) * 1024u, P, c2row);
                }
            }
            if constexpr (T == 0) {                                     // the h the stage before produced (units 0..95) becomes its layer's operand
                static_for<3>([&](auto pc) {
                    constexpr int pt = decltype(pc)::value;
                    if constexpr (KS > 3 ? pt == i : i == 0) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) w.own[PREV][4 * pt + e] = w.nxt[4 * pt + e];
                    }
                });
            }
            if constexpr (MIXED != 0 && T == 0) {
                // the mixed operand, built ONCE per stage (it is the same for all 13 super-tiles; per super-tile it cost ~14 moves and perms, and at the
                // power limit every instruction not issued is time) when super-tile 0 needs it: super-tile 12 of the stage before finished just above.  Slots
                // (own_hi, own_hi | own_lo, in_hi | in_hi, in_lo | 1, 1) against the record's (w_hi, w_lo | w_hi, v_hi | v_lo, v_hi | b_hi, b_lo)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    unsigned in_hl;                                     // (hi, lo) of input unit 96 + g / of feature g
                    if constexpr (L0) in_hl = x0p[hh];
                    else in_hl = w.m12[LAYER - 1][hh][1];
                    unsigned own_hh = w.m12[LAYER][hh][0], own_hl = w.m12[LAYER][hh][1];
                    asm volatile("" : "+v"(own_hh), "+v"(own_hl), "+v"(in_hl));      // opaque scalars: hipcc otherwise widens the first one into a 16-byte load that keeps m12 in scratch
                    mx[hh] = uintx4{own_hh, hi_lo(own_hl, in_hl), in_hl, one2};
                    if constexpr (L0) mx2[hh] = uintx4{x1a[hh], x1b[hh], 0u, 0u};
                }
            }
            constexpr bool WITH_B_NEXT = T + 1 < NTILE - 1;
            if constexpr (PF_OUT && i == KS - 1) load_a<K::rec_off(0), WITH_B_NEXT, K::mixed(0)>(a[KS & 1], lds_base + unsigned((w.slot + 1) & (NS - 1)) * SLOT_BYTES + lane16);
            wait_a<(i + 1 < KS ? a_reads(WITH_B, K::mixed(i + 1 < KS ? i + 1 : i)) : (PF_OUT ? a_reads(WITH_B_NEXT, K::mixed(0)) : 0))>(ai);
            // the products: per product the 2 x 2 (row half x window half) tiles of the super-tile, four independent accumulators; each MFMA is
            // followed by its share of super-tile P's cell update (16 cycles hide about two VALU issues)
            constexpr int C0 = DM16Q_PRE + NMF * i;
#define DM_MF(AOP, BOP, Q, NO)                                                                                              \
            d[Q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AOP, BOP, (i == 0 && (NO) == 0) ? z4 : d[Q], 0, 0, 0);              \
            asm volatile(DM16Q_AFTER_MFMA : "+v"(d[Q]) : "v"(AOP), "v"(BOP));      /* the sources stay live past the MFMA: hipcc otherwise lets vDst overlap a dying SrcA */
#define DM_MI(AOP, BOP, Q)                                                                                                  \
            di[Q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(intx4, AOP), __builtin_bit_cast(intx4, BOP), i == 0 ? zi4 : di[Q], 0, 0, 0); \
            asm volatile(DM16Q_AFTER_MFMA : "+v"(di[Q]) : "v"(AOP), "v"(BOP));
#define DM_CELLQ(N_) if constexpr (KS > 1 && i < KS - 1) DM_CHUNK(C0 + (N_))
            if constexpr (MIXED != 0) {
                // all three products of the left-over slots in one MFMA per 16x16 tile (layer 0: a second one for features 4..6); the last
                // k32-step of a super-tile, no cell chunks under it
                const halfx8 b0 = as_h8(mx[0]), b1 = as_h8(mx[1]);
                DM_MF(ai.hiA, b0, 0, 0)
                DM_MF(ai.hiA, b1, 2, 0)
                if constexpr (WITH_B) { DM_MF(ai.hiB, b0, 1, 0) DM_MF(ai.hiB, b1, 3, 0) }
                if constexpr (MIXED == 2) {
                    const halfx8 e0 = as_h8(mx2[0]), e1 = as_h8(mx2[1]);
                    DM_MF(ai.loA, e0, 0, 1)
                    DM_MF(ai.loA, e1, 2, 1)
                    if constexpr (WITH_B) { DM_MF(ai.loB, e0, 1, 1) DM_MF(ai.loB, e1, 3, 1) }
                }
            } else {
                constexpr int t = K::opnd(i);
                halfx8 bh[2], bl[2];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    if constexpr (K::is_own(i)) { bh[hh] = as_h8(own[quad(t, hh, 0)]); bl[hh] = as_h8(own[quad(t, hh, 1)]); }
                    else { bh[hh] = as_h8(inp[quad(t, hh, 0)]); bl[hh] = as_h8(inp[quad(t, hh, 1)]); }
                }
                if constexpr (I8) {
                    // a_hi w_hi in f16, then both cross terms of the 32 units of this k32-step in one int8 MFMA per tile: A bytes (w_hi8, w_lo8) x B bytes (lo8, hi8)
                    DM_MF(ai.hiA, bh[0], 0, 0) DM_CELLQ(0);
                    DM_MF(ai.hiA, bh[1], 2, 0) DM_CELLQ(1);
                    if constexpr (WITH_B) { DM_MF(ai.hiB, bh[0], 1, 0) DM_CELLQ(2); DM_MF(ai.hiB, bh[1], 3, 0) DM_CELLQ(3); }
                    DM_MI(ai.loA, bl[0], 0) DM_CELLQ(WITH_B ? 4 : 2);
                    DM_MI(ai.loA, bl[1], 2) DM_CELLQ(WITH_B ? 5 : 3);
                    if constexpr (WITH_B) { DM_MI(ai.loB, bl[0], 1) DM_CELLQ(6); DM_MI(ai.loB, bl[1], 3) DM_CELLQ(7); }
                } else {
                // the snake order (profiles/r05/ablate_sched.txt: 1.328 against 1.337 / 1.339 ms): every MFMA changes ONE operand against the one before it
                // (row half or window half), also across the products.  Each accumulator Q still receives product 0 (a_hi w_hi), then 1 (a_hi w_lo), then 2
                // (a_lo w_hi) of the same operands, so the sums are what the product-major order gave, bit for bit
                DM_MF(ai.hiA, bh[0], 0, 0) DM_CELLQ(0);
                if constexpr (WITH_B) { DM_MF(ai.hiB, bh[0], 1, 0) DM_CELLQ(1); DM_MF(ai.hiB, bh[1], 3, 0) DM_CELLQ(2); }
                DM_MF(ai.hiA, bh[1], 2, 0) DM_CELLQ(WITH_B ? 3 : 1);
                DM_MF(ai.loA, bh[1], 2, 1) DM_CELLQ(WITH_B ? 4 : 2);
                if constexpr (WITH_B) { DM_MF(ai.loB, bh[1], 3, 1) DM_CELLQ(5); DM_MF(ai.loB, bh[0], 1, 1) DM_CELLQ(6); }
                DM_MF(ai.loA, bh[0], 0, 1) DM_CELLQ(WITH_B ? 7 : 3);
                DM_MF(ai.hiA, bl[0], 0, 2) DM_CELLQ(WITH_B ? 8 : 4);
                if constexpr (WITH_B) { DM_MF(ai.hiB, bl[0], 1, 2) DM_CELLQ(9); DM_MF(ai.hiB, bl[1], 3, 2) DM_CELLQ(10); }
                DM_MF(ai.hiA, bl[1], 2, 2) DM_CELLQ(WITH_B ? 11 : 5);
                }
            }
#undef DM_MF
#undef DM_MI
#undef DM_CELLQ
        });
#undef DM_CHUNK
#ifdef DM16Q_ABL_PAIRBAR      // timing only, on the TWO-slot ring (the weights of an odd super-tile may not have landed): what one barrier and one DMA wait per two super-tiles
                              // could save at most - measured before the four-slot ring was built (profiles/edges/README.md)
        if constexpr ((T & 1) == 0) {
#else
        if constexpr (EDGE) {
#endif
#ifndef DM16Q_ABL_NOVMWAIT
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // this wave's pieces of the next group have landed ...
#endif
#ifndef DM16Q_ABL_NOBAR
        __builtin_amdgcn_s_barrier();                                   // ... everyone's; and everyone is done with this group's slots
#endif
        }
        w.slot = (w.slot + 1) & (NS - 1);
    });
}

// work item = (tile of 128 windows, direction); partial logits per direction, lstmhead::head_finish_kernel adds them.
// MM: 0 DM_PREC_F16X3 (three f16 products), 1 DM_PREC_F16I8 (int8 cross terms, p.wpack = the int8 pack, p.i8s = its fold scales)
template <int MM>
__global__ __launch_bounds__(THREADS, 1) void bilstm_f16q_kernel(const Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds16q[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int grp = lane >> 4, n16 = lane & 15;
    const unsigned lane16 = unsigned(lane) * 16u;
    const unsigned lds_base = (unsigned)(size_t)lds16q;
    const unsigned c2_wave = lds_base + unsigned(ring_slots(MM)) * SLOT_BYTES + unsigned(wave) * C2_WAVE_BYTES + lane16;
    const unsigned one2 = grp == 0 ? 0x3C003C00u : 0u;           // f16 (1.0, 1.0): the slots of lane group 0 that meet (bias hi, bias lo) in the mixed k32-step
    const int nwork = 2 * p.ntiles;
    for (int work = blockIdx.x; work < nwork; work += gridDim.x) {
        const int tile = work >> 1, dir = work & 1;
        const long long tile0 = (long long)tile * TILE_M;
        const long long w_out = tile0 + wave * 32 + n16;          // window of window half 0; half 1: + 16
        long long wi0 = w_out, wi1 = w_out + 16;
        if (wi0 > p.n - 1) wi0 = p.n - 1;
        if (wi1 > p.n - 1) wi1 = p.n - 1;
        const float* xwin0 = p.x + (p.widx ? (long long)p.widx[wi0] : wi0) * p.xstride;
        const float* xwin1 = p.x + (p.widx ? (long long)p.widx[wi1] : wi1) * p.xstride;
        const unsigned char* wdir = p.wpack + size_t(dir) * WEIGHT_BYTES_DIR;

        WaveState w;
#pragma unroll
        for (int l = 0; l < 3; ++l) {
#pragma unroll
            for (int q = 0; q < 12; ++q) w.own[l][q] = uintx4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) w.m12[l][hh][0] = w.m12[l][hh][1] = 0u;      // h = 0
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) w.nxt[q] = uintx4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < NTILE; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) w.c2reg[t][q] = w.c1reg[t][q] = 0.0f;
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) w.acc[t][q] = floatx4{0.f, 0.f, 0.f, 0.f};      // acc[2] = "super-tile 12 of the stage before the first": h = 0, c = 0
        w.cp.hi01 = w.cp.hi23 = w.cp.lo01 = w.cp.lo23 = 0u;
        if constexpr (MM == 1) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) w.acci[t][q] = intx4{0, 0, 0, 0};
#pragma unroll
            for (int l = 0; l < 3; ++l)
#pragma unroll
                for (int k = 0; k < 2; ++k) w.i8s[l][k] = floatx2{p.i8s[(dir * 3 + l) * 4 + 2 * k], p.i8s[(dir * 3 + l) * 4 + 2 * k + 1]};
            w.cp.kmagic = floatx2{I8_MAGIC, I8_MAGIC};
            w.cp.khi = floatx2{I8_HI_SCALE, I8_HI_SCALE};
            w.cp.klo = floatx2{I8_LO_SCALE, I8_LO_SCALE};
            w.cp.i01 = w.cp.i23 = 0u;
        }
        w.slot = 0;
        __syncthreads();                                          // the previous work item is done with the ring and the cell rows
        {   // zero cell state of layer 0 (this lane's rows)
            const floatx4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < NTILE; ++t) {
                asm volatile("ds_write_b128 %0, %1" :: "v"(c2_wave + unsigned(t * 1024)), "v"(z4) : "memory");
                if constexpr (MM == 1) asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(c2_wave + unsigned(t * 1024)), "v"(z4), "i"(C2_LAYER_BYTES) : "memory");
            }
        }
        {   // layer 0, super-tile 0 -> slot 0 (step 0: only its mixed record); the four-slot ring runs two super-tiles ahead: super-tile 1 -> slot 1
            using K0 = StageKind<0, true>;
            stage_tile<K0::DMA_BYTES>(wdir + K0::DMA_OFF, lds_base + K0::DMA_OFF, wave_s, lane16);
            if constexpr (ring_slots(MM) == 4) stage_tile<K0::DMA_BYTES>(wdir + (K0::TILE_BYTES + K0::DMA_OFF), lds_base + (SLOT_BYTES + K0::DMA_OFF), wave_s, lane16);
        }
        {
            const int row = dir == 0 ? 0 : WIN - 1;
            const int f1 = 4 + grp < NFEAT ? 4 + grp : NFEAT - 1;
            w.xf[0][0] = xwin0[row * NFEAT + grp]; w.xf[0][1] = xwin0[row * NFEAT + f1];
            w.xf[1][0] = xwin1[row * NFEAT + grp]; w.xf[1][1] = xwin1[row * NFEAT + f1];
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();

#define DM_STAGE(LAYER, FIRST, S_) run_stage<LAYER, FIRST, MM>(p, w, lds_base, c2_wave, wdir, dir, S_, xwin0, xwin1, wave_s, lane16, grp, one2)
        DM_STAGE(0, true, 0);
        DM_STAGE(1, true, 0);
        DM_STAGE(2, true, 0);
        for (int s = 1; s < LIVE; ++s) {
            DM_STAGE(0, false, s);
            DM_STAGE(1, false, s);
            DM_STAGE(2, false, s);
        }
#undef DM_STAGE
        // ---- tail: super-tile 12 of the last stage (layer 2), then the head on the final h of layer 2 ----
        {
            float c2row[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) c2row[q] = w.c2reg[NTILE - 1][q];
            w.cp.template all<MM, 0>(w.acc[2], w.acci[2], w.i8s[2], c2row, true);
            w.m12[2][0][1] = lo_lo(w.cp.hi01, w.cp.lo01);
            w.m12[2][1][1] = lo_lo(w.cp.hi23, w.cp.lo23);
#pragma unroll
            for (int q = 0; q < 12; ++q) w.own[2][q] = w.nxt[q];
        }
        // logits(dir) = h_final(dir) . W[dir*100 + u][class]; h = hi + lo (the operand halves, 22 bits); this lane: units 8S + 4 rh + grp
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            float hsum0 = 0.0f, hsum1 = 0.0f;
            static_for<NTILE>([&](auto Sc) {
                constexpr int S = decltype(Sc)::value;
                unsigned hi, lo;
                if constexpr (S < 12) { hi = w.own[2][quad(S >> 2, hh, 0)][S & 3]; lo = w.own[2][quad(S >> 2, hh, 1)][S & 3]; }
                else { hi = w.m12[2][hh][1]; lo = w.m12[2][hh][1] >> 16; }      // (hi, lo) of unit 96 + g in one register
                const halfx2 h2 = __builtin_bit_cast(halfx2, hi), l2 = __builtin_bit_cast(halfx2, lo);
#pragma unroll
                for (int rh = 0; rh < (S < 12 ? 2 : 1); ++rh) {
                    const float h = (float)h2[rh] + (float)l2[rh];
                    const float* wo = p.hpack + (dir * HID + 8 * S + 4 * rh + grp) * 2;
                    hsum0 = fmaf(h, wo[0], hsum0);
                    hsum1 = fmaf(h, wo[1], hsum1);
                }
            });
            hsum0 += __shfl_xor(hsum0, 16, 64);
            hsum1 += __shfl_xor(hsum1, 16, 64);
            hsum0 += __shfl_xor(hsum0, 32, 64);
            hsum1 += __shfl_xor(hsum1, 32, 64);
            if (lane < 16) {
                float* pl = p.plogit + (size_t(dir) * p.ntiles * TILE_M + size_t(w_out + 16 * hh)) * 2;
                pl[0] = hsum0;
                pl[1] = hsum1;
            }
        }
    }
}

}  // namespace lstm16q
