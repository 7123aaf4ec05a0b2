// Microbenchmark of the PLL walker's lane-block transition on gfx950 (k_pll.hip WL_LB):
// the issue rules of one wave alone on its CU with 256 VGPRs, as the walker runs, and
// the transition itself in the orders tried.  Device cycles (s_memtime) per body,
// kUnroll bodies per loop trip, kTrips trips, the empty loop's share subtracted.
//   hipcc --offload-arch=gfx950 -O3 walk_trans.hip -o walk_trans && ./walk_trans
// Groups: D* a VALU result read 1 / 2 / 3 slots later; B* v_cmp -> s_cbranch_vccz with
// 0-3 independent instructions between; M* how many independent VALU / LDS
// instructions v_mul_lo_u32 hides before v_add3_u32 waits; L* the issue cost of
// ds_write_b32 / ds_read_b128 between VALU instructions; S* SALU beside VALU;
// T* the transition: T0 as the parent commit wrote it, T1-T14 the orders tried,
// TN without the interval test (the bound, k_pll_walk VAR 256).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>

constexpr int kUnroll = 4;
constexpr int kTrips = 50000;      // 200 000 bodies

// a0-a7: VALU scratch; x / xn: the two offsets; e0y, e0w, e1w, n0x, n0y, sxn: entry
// fields; xs / ln: LDS addresses of the xbuf write and the entry reads; v100-v107:
// the entry registers that the reads refill.  n0y = ~0: no lane-block has an event
// (the branch behind the transition is always taken, as in VAR 224 / 256).
#define TR_KERNEL(NAME, BODY)                                                                                     \
    __global__ void __launch_bounds__(64) NAME(uint32_t* out, unsigned long long* clk, uint32_t n0yv)              \
    {                                                                                                             \
        __shared__ uint4 lds[1024];                                                                               \
        const uint32_t lane = threadIdx.x;                                                                        \
        lds[lane] = make_uint4(lane, 1u, 2u, 3u);                                                                 \
        lds[512 + lane] = make_uint4(lane, 5u, 6u, 7u);                                                           \
        __syncthreads();                                                                                          \
        asm volatile("" ::: "v255");                                                                              \
        uint32_t a0 = lane, a1 = lane + 1, a2 = lane + 2, a3 = lane + 3, a4 = 4, a5 = 5, a6 = 6, a7 = 7;          \
        uint32_t x = 1000u + lane, xn = 7u, t = 0, t2 = 0, off = 0, acc = 0;                                      \
        uint32_t e0y = 900u, e0w = 100u, e1w = 5000u, n0x = 3u * lane, n0y = n0yv, sxn = lane;                    \
        uint32_t xs = (uint32_t)(uintptr_t)&lds[0] + 12288u + lane * 4u;                                          \
        uint32_t ln = (uint32_t)(uintptr_t)&lds[0] + lane * 16u;                                                  \
        uint32_t kb = 11u, d = 13u, s0 = 1u, s1 = 2u, s2 = 3u, s3 = 4u, n = kTrips;                               \
        unsigned long long t0, t1;                                                                                \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");                                \
        asm volatile("1:\n\t" BODY BODY BODY BODY                                                                 \
                     "s_sub_u32 %[n], %[n], 1\n\t"                                                                \
                     "s_cmp_lg_u32 %[n], 0\n\t"                                                                   \
                     "s_cbranch_scc1 1b\n\t"                                                                      \
                     "s_waitcnt lgkmcnt(0)"                                                                       \
                     : [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2), [a3] "+v"(a3), [a4] "+v"(a4), [a5] "+v"(a5),  \
                       [a6] "+v"(a6), [a7] "+v"(a7), [x] "+v"(x), [xn] "+v"(xn), [t] "+v"(t), [t2] "+v"(t2),      \
                       [off] "+v"(off), [acc] "+v"(acc), [kb] "+s"(kb), [d] "+s"(d), [s0] "+s"(s0),               \
                       [s1] "+s"(s1), [s2] "+s"(s2), [s3] "+s"(s3), [n] "+s"(n)                                   \
                     : [e0y] "v"(e0y), [e0w] "v"(e0w), [e1w] "v"(e1w), [n0x] "v"(n0x), [n0y] "v"(n0y),            \
                       [sxn] "v"(sxn), [xs] "v"(xs), [ln] "v"(ln)                                                 \
                     : "scc", "vcc", "memory", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107");   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");                                \
        out[lane] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + x + xn + t + t2 + off + acc + kb + d + s0 + s1 + s2 + \
                    s3;                                                                                           \
        if (lane == 0) *clk = t1 - t0;                                                                            \
    }

#define VI(K) "v_add_u32 %[a" #K "], %[e0y], %[e0w]\n\t"                 /* independent VALU */
#define VD(K, J) "v_add_u32 %[a" #K "], %[a" #J "], %[e0w]\n\t"          /* a_K = a_J + .. */
#define SI(K) "s_add_u32 %[s" #K "], %[kb], %[d]\n\t"                    /* independent SALU */
#define DW "ds_write_b32 %[xs], %[x] offset:256\n\t"
#define DR0 "ds_read_b128 v[100:103], %[ln]\n\t"
#define DR1 "ds_read_b128 v[104:107], %[ln] offset:8192\n\t"
#define LW "s_waitcnt lgkmcnt(0)\n\t"

TR_KERNEL(k_empty, "")
// eight VALU instructions: independent; one chain; two / three chains interleaved
TR_KERNEL(k_i8, VI(0) VI(1) VI(2) VI(3) VI(4) VI(5) VI(6) VI(7))
TR_KERNEL(k_d1, VD(0, 0) VD(0, 0) VD(0, 0) VD(0, 0) VD(0, 0) VD(0, 0) VD(0, 0) VD(0, 0))
TR_KERNEL(k_d2, VD(0, 0) VD(1, 1) VD(0, 0) VD(1, 1) VD(0, 0) VD(1, 1) VD(0, 0) VD(1, 1))
TR_KERNEL(k_d3, VD(0, 0) VD(1, 1) VD(2, 2) VD(0, 0) VD(1, 1) VD(2, 2) VD(0, 0) VD(1, 1))
// the test's own dependent pairs: sub -> sub clamp, sub clamp -> min, min -> or
TR_KERNEL(k_d1c, "v_sub_u32 %[t], %[x], %[e0w]\n\tv_sub_u32_e64 %[t], %[t], %[e1w] clamp\n\t"
                 "v_min_u32 %[t], %[t], %[off]\n\tv_or_b32 %[acc], %[acc], %[t]\n\t")
// v_cmp -> k independent VALU -> s_cbranch_vccz (taken: n0y = ~0), and the k alone
#define CMPV "v_cmp_gt_u32_e32 vcc, %[xn], %[n0y]\n\t"
#define BRZ "s_cbranch_vccz 2f\n\tv_add_u32 %[a7], 1, %[a7]\n2:\n\t"
TR_KERNEL(k_b0, CMPV BRZ)
TR_KERNEL(k_b1, CMPV VI(0) BRZ)
TR_KERNEL(k_b2, CMPV VI(0) VI(1) BRZ)
TR_KERNEL(k_b3, CMPV VI(0) VI(1) VI(2) BRZ)
TR_KERNEL(k_b4, CMPV VI(0) VI(1) VI(2) VI(3) BRZ)
TR_KERNEL(k_b2l, CMPV DR0 DR1 BRZ)
TR_KERNEL(k_b1s, CMPV SI(0) BRZ)
TR_KERNEL(k_b2s, CMPV SI(0) SI(1) BRZ)
// v_add3 -> v_cmp with 0 / 1 independent VALU between (the chain's second hop)
#define ADD3 "v_add3_u32 %[xn], %[n0x], %[kb], %[t2]\n\t"
TR_KERNEL(k_ac0, ADD3 CMPV BRZ)
TR_KERNEL(k_ac1, ADD3 VI(0) CMPV BRZ)
TR_KERNEL(k_ac2, ADD3 VI(0) VI(1) CMPV BRZ)
// v_mul_lo_u32 (reads the previous v_add3: a serial chain) -> k fillers -> v_add3
#define MUL "v_mul_lo_u32 %[t2], %[xn], %[sxn]\n\t"
TR_KERNEL(k_m0, MUL ADD3)
TR_KERNEL(k_m1, MUL VI(0) ADD3)
TR_KERNEL(k_m2, MUL VI(0) VI(1) ADD3)
TR_KERNEL(k_m3, MUL VI(0) VI(1) VI(2) ADD3)
TR_KERNEL(k_m4, MUL VI(0) VI(1) VI(2) VI(3) ADD3)
TR_KERNEL(k_m5, MUL VI(0) VI(1) VI(2) VI(3) VI(4) ADD3)
TR_KERNEL(k_m6, MUL VI(0) VI(1) VI(2) VI(3) VI(4) VI(5) ADD3)
TR_KERNEL(k_m8, MUL VI(0) VI(1) VI(2) VI(3) VI(4) VI(5) VI(6) VI(7) ADD3)
TR_KERNEL(k_m2w, MUL VI(0) DW VI(1) ADD3 LW)
TR_KERNEL(k_m2r, MUL VI(0) DR0 VI(1) ADD3 LW)
TR_KERNEL(k_m2wr, MUL VI(0) DW DR0 VI(1) ADD3 LW)
TR_KERNEL(k_m2lw, MUL VI(0) VI(1) ADD3 LW)
// LDS issue cost between independent VALU instructions (each body drains the queue)
TR_KERNEL(k_l0, VI(0) VI(1) VI(2) VI(3) LW)
TR_KERNEL(k_lw, VI(0) VI(1) DW VI(2) VI(3) LW)
TR_KERNEL(k_lr, VI(0) VI(1) DR0 VI(2) VI(3) LW)
TR_KERNEL(k_lrr, VI(0) VI(1) DR0 DR1 VI(2) VI(3) LW)
TR_KERNEL(k_lr_r, VI(0) DR0 VI(1) VI(2) DR1 VI(3) LW)
TR_KERNEL(k_lwrr, VI(0) DW VI(1) DR0 VI(2) DR1 VI(3) LW)
// the same with the LDS queue left to run (issue cost alone; lgkmcnt never waited on)
TR_KERNEL(k_nw, VI(0) VI(1) DW VI(2) VI(3))
TR_KERNEL(k_nr, VI(0) VI(1) DR0 VI(2) VI(3))
TR_KERNEL(k_nrr, VI(0) VI(1) DR0 DR1 VI(2) VI(3))
TR_KERNEL(k_nwrr, VI(0) VI(1) DW DR0 DR1 VI(2) VI(3))
TR_KERNEL(k_nsw, SI(0) SI(1) DW SI(2) SI(3))
// SALU beside VALU: alternating, grouped, and each reading the other's result
TR_KERNEL(k_s4, SI(0) SI(1) SI(2) SI(3))
TR_KERNEL(k_v4, VI(0) VI(1) VI(2) VI(3))
TR_KERNEL(k_vs, VI(0) SI(0) VI(1) SI(1) VI(2) SI(2) VI(3) SI(3))
TR_KERNEL(k_vvss, VI(0) VI(1) VI(2) VI(3) SI(0) SI(1) SI(2) SI(3))
TR_KERNEL(k_sv_dep, "s_add_u32 %[s0], %[s0], 1\n\tv_add_u32 %[a0], %[s0], %[a0]\n\t"
                    "s_add_u32 %[s0], %[s0], 1\n\tv_add_u32 %[a0], %[s0], %[a0]\n\t")
TR_KERNEL(k_vs_dep, "v_add_u32 %[a0], 1, %[a0]\n\tv_readfirstlane_b32 %[s0], %[a0]\n\ts_add_u32 %[s1], %[s0], %[s1]\n\t"
                    "v_add_u32 %[a0], 1, %[a0]\n\tv_readfirstlane_b32 %[s0], %[a0]\n\ts_add_u32 %[s1], %[s0], %[s1]\n\t")

// ---- the transition.  The multiply reads the previous body's offsets (xn), standing
// for the chain through the VCCZ branch and the repair loop that the walker has.
#define T_MUL "v_mul_lo_u32 %[t2], %[xn], %[sxn]\n\t"
#define T_OFF "v_sub_u32_e64 %[off], %[x], %[e0y] clamp\n\t"
#define T_SUB "v_sub_u32 %[t], %[x], %[e0w]\n\t"
#define T_CLP "v_sub_u32_e64 %[t], %[t], %[e1w] clamp\n\t"
#define T_MIN "v_min_u32 %[t], %[t], %[off]\n\t"
#define T_OR "v_or_b32 %[acc], %[acc], %[t]\n\t"
#define T_BR "s_cbranch_vccz 2f\n\tv_add_u32 %[a7], 1, %[a7]\n2:\n\t"
// T0: the parent's order (all six fillers in the multiply's shadow, both reads behind the compare)
TR_KERNEL(k_t0, T_MUL T_OFF T_SUB T_CLP T_MIN T_OR DW ADD3 CMPV DR0 DR1 T_BR)
// TN: no test (VAR 256)
TR_KERNEL(k_tn, T_MUL DW ADD3 CMPV DR0 DR1 T_BR)
// T1: no filler behind the one it reads; min between add3 and compare, or + E1 read behind the compare
TR_KERNEL(k_t1, T_MUL T_SUB T_OFF DW T_CLP DR0 ADD3 T_MIN CMPV T_OR DR1 T_BR)
// T2: as T1 with the LDS write behind the compare too
TR_KERNEL(k_t2, T_MUL T_SUB T_OFF T_CLP DR0 ADD3 T_MIN CMPV T_OR DW DR1 T_BR)
// T3: the shadow holds the two subtracts, the write and the clamp; min and or behind the compare
TR_KERNEL(k_t3, T_MUL T_SUB T_OFF DW T_CLP ADD3 CMPV T_MIN DR0 T_OR DR1 T_BR)
// T4: the whole test behind the compare (the shadow holds the write only)
TR_KERNEL(k_t4, T_MUL DW ADD3 CMPV T_SUB T_OFF T_CLP DR0 T_MIN DR1 T_OR T_BR)
// T5: the parent's order with the fillers un-chained only (sub, off, write, clamp, min, or)
TR_KERNEL(k_t5, T_MUL T_SUB T_OFF DW T_CLP T_MIN T_OR ADD3 CMPV DR0 DR1 T_BR)
// T6: three fillers in the shadow, the rest split around the compare, the reads last
TR_KERNEL(k_t6, T_MUL T_SUB T_OFF T_CLP ADD3 DW CMPV T_MIN T_OR DR0 DR1 T_BR)
// TN2: no test, the write behind the compare too
TR_KERNEL(k_tn2, T_MUL ADD3 CMPV DW DR0 DR1 T_BR)
// T7-T13: the write and both reads behind the compare; 3 / 2 / 1 / 0 of the test's five there
TR_KERNEL(k_t7, T_MUL T_SUB T_CLP ADD3 CMPV T_OFF T_MIN T_OR DW DR0 DR1 T_BR)
TR_KERNEL(k_t8, T_MUL T_SUB T_CLP ADD3 CMPV DW T_OFF T_MIN T_OR DR0 DR1 T_BR)
TR_KERNEL(k_t9, T_MUL T_SUB T_OFF T_CLP ADD3 CMPV T_MIN T_OR DW DR0 DR1 T_BR)
TR_KERNEL(k_t10, T_MUL T_SUB T_OFF T_CLP T_MIN ADD3 CMPV T_OR DW DR0 DR1 T_BR)
TR_KERNEL(k_t11, T_MUL T_OFF T_SUB T_CLP T_MIN T_OR ADD3 CMPV DW DR0 DR1 T_BR)
TR_KERNEL(k_t12, T_MUL T_SUB T_OFF T_CLP ADD3 CMPV DW DR0 DR1 T_MIN T_OR T_BR)
TR_KERNEL(k_t13, T_MUL T_SUB T_CLP ADD3 CMPV T_OFF DR0 T_MIN DW T_OR DR1 T_BR)
// T14: the test in front of the multiply (nothing in its shadow), LDS behind the compare
TR_KERNEL(k_t14, T_SUB T_OFF T_CLP T_MIN T_OR T_MUL ADD3 CMPV DW DR0 DR1 T_BR)

int main()
{
    uint32_t* dout;
    unsigned long long* dclk;
    if (hipMalloc(&dout, 256) != hipSuccess || hipMalloc(&dclk, 8) != hipSuccess) return 1;
    double empty = 0;
    auto run = [&](auto kern, const char* name, bool base = false) {
        for (int rep = 0; rep < 2; rep++) hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, 0, dout, dclk, ~0u);
        if (hipDeviceSynchronize() != hipSuccess) {
            printf("%s: launch failed\n", name);
            exit(1);
        }
        unsigned long long c = 0;
        if (hipMemcpy(&c, dclk, 8, hipMemcpyDeviceToHost) != hipSuccess) exit(1);
        const double per = (double)c / ((double)kUnroll * kTrips);
        if (base) empty = per;
        printf("%-58s %7.2f cycles per body (%7.2f beyond the empty loop)\n", name, per, per - empty);
    };
    for (int r = 0; r < 5; r++) {
        printf("---- round %d\n", r + 1);
        run(k_empty, "E   empty loop (3 SALU per 4 bodies)", true);
        run(k_i8, "I8  8 independent v_add");
        run(k_d1, "D1  8 v_add, each reads the one before");
        run(k_d2, "D2  8 v_add, each reads the one 2 before");
        run(k_d3, "D3  8 v_add, each reads the one 3 before");
        run(k_d1c, "D1c sub -> sub clamp -> min -> or (the test's chain)");
        run(k_b0, "B0  v_cmp, s_cbranch_vccz (taken)");
        run(k_b1, "B1  v_cmp, 1 VALU, s_cbranch_vccz");
        run(k_b2, "B2  v_cmp, 2 VALU, s_cbranch_vccz");
        run(k_b3, "B3  v_cmp, 3 VALU, s_cbranch_vccz");
        run(k_b4, "B4  v_cmp, 4 VALU, s_cbranch_vccz");
        run(k_b2l, "B2l v_cmp, 2 ds_read_b128, s_cbranch_vccz");
        run(k_b1s, "B1s v_cmp, 1 SALU, s_cbranch_vccz");
        run(k_b2s, "B2s v_cmp, 2 SALU, s_cbranch_vccz");
        run(k_ac0, "AC0 v_add3, v_cmp, branch");
        run(k_ac1, "AC1 v_add3, 1 VALU, v_cmp, branch");
        run(k_ac2, "AC2 v_add3, 2 VALU, v_cmp, branch");
        run(k_m0, "M0  v_mul_lo, v_add3 (serial chain)");
        run(k_m1, "M1  v_mul_lo, 1 VALU, v_add3");
        run(k_m2, "M2  v_mul_lo, 2 VALU, v_add3");
        run(k_m3, "M3  v_mul_lo, 3 VALU, v_add3");
        run(k_m4, "M4  v_mul_lo, 4 VALU, v_add3");
        run(k_m5, "M5  v_mul_lo, 5 VALU, v_add3");
        run(k_m6, "M6  v_mul_lo, 6 VALU, v_add3");
        run(k_m8, "M8  v_mul_lo, 8 VALU, v_add3");
        run(k_m2lw, "M2+ M2 and s_waitcnt lgkmcnt(0)");
        run(k_m2w, "M2w M2+ with a ds_write_b32 between the two VALU");
        run(k_m2r, "M2r M2+ with a ds_read_b128 between the two VALU");
        run(k_m2wr, "M2wr M2+ with both between the two VALU");
        run(k_l0, "L0  4 VALU, s_waitcnt lgkmcnt(0)");
        run(k_lw, "Lw  L0 with a ds_write_b32 in the middle");
        run(k_lr, "Lr  L0 with a ds_read_b128 in the middle");
        run(k_lrr, "Lrr L0 with two ds_read_b128 in the middle");
        run(k_lr_r, "Lr_r L0 with two ds_read_b128, a VALU pair between");
        run(k_lwrr, "Lwrr L0 with write, read, read, one VALU between each");
        run(k_nw, "Nw  4 VALU, a ds_write_b32 in the middle, no wait");
        run(k_nr, "Nr  4 VALU, a ds_read_b128 in the middle, no wait");
        run(k_nrr, "Nrr 4 VALU, two ds_read_b128 in the middle, no wait");
        run(k_nwrr, "Nwrr 4 VALU, write + two reads in the middle, no wait");
        run(k_nsw, "Nsw 4 SALU, a ds_write_b32 in the middle, no wait");
        run(k_s4, "S4  4 independent s_add");
        run(k_v4, "V4  4 independent v_add");
        run(k_vs, "VS  v_add, s_add alternating, 4 each");
        run(k_vvss, "VVSS 4 v_add then 4 s_add");
        run(k_sv_dep, "SVd 2 x (s_add, v_add reading it)");
        run(k_vs_dep, "VSd 2 x (v_add, v_readfirstlane, s_add reading it)");
        run(k_t0, "T0  transition, the parent's order");
        run(k_tn, "TN  transition without the test (bound)");
        run(k_t1, "T1  sub off W clamp R0 | add3 min cmp or R1");
        run(k_t2, "T2  sub off clamp R0 | add3 min cmp or W R1");
        run(k_t3, "T3  sub off W clamp | add3 cmp min R0 or R1");
        run(k_t4, "T4  W | add3 cmp sub off clamp R0 min R1 or");
        run(k_t5, "T5  sub off W clamp min or | add3 cmp R0 R1");
        run(k_t6, "T6  sub off clamp | add3 W cmp min or R0 R1");
        run(k_tn2, "TN2 no test: add3 cmp W R0 R1");
        run(k_t7, "T7  sub clamp | add3 cmp off min or W R0 R1");
        run(k_t8, "T8  sub clamp | add3 cmp W off min or R0 R1");
        run(k_t9, "T9  sub off clamp | add3 cmp min or W R0 R1");
        run(k_t10, "T10 sub off clamp min | add3 cmp or W R0 R1");
        run(k_t11, "T11 off sub clamp min or | add3 cmp W R0 R1");
        run(k_t12, "T12 sub off clamp | add3 cmp W R0 R1 min or");
        run(k_t13, "T13 sub clamp | add3 cmp off R0 min W or R1");
        run(k_t14, "T14 sub off clamp min or mul add3 cmp W R0 R1");
    }
    return 0;
}
