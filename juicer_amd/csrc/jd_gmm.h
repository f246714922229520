// jd_gmm.h - the companion scoring kernels of juicer_amd (included by jd_device.hip; gfx950 only):
// HTKFlatModels::calcGMMOutput + logAdd (src/HTKFlatModels.cpp:226-293) for every tied state of every frame of a
// likelihood table - jd_gmm_kernel39 (D = 39: two frames per lane, packed fp32, the reference's roundings) and the
// generic jd_gmm_kernel - with the bit-exact replicas of glibc's expf and log they need.
#pragma once

// glibc 2.35 expf (sysdeps/ieee754/flt-32/e_expf.c, ARM optimized-routines
// algorithm): N=32 table + cubic in double, rounded once to float.  Replicated
// so that device logAdd equals the host libm result bit for bit (verified on
// the host for all 1.2e8 floats in [-18.5, -1e-3]: tests/test_expf.py, through jd_debug_expf).
#define JD_EXP2F_TAB                                                                              \
    0x3ff0000000000000ULL, 0x3fefd9b0d3158574ULL, 0x3fefb5586cf9890fULL, 0x3fef9301d0125b51ULL,   \
    0x3fef72b83c7d517bULL, 0x3fef54873168b9aaULL, 0x3fef387a6e756238ULL, 0x3fef1e9df51fdee1ULL,   \
    0x3fef06fe0a31b715ULL, 0x3feef1a7373aa9cbULL, 0x3feedea64c123422ULL, 0x3feece086061892dULL,   \
    0x3feebfdad5362a27ULL, 0x3feeb42b569d4f82ULL, 0x3feeab07dd485429ULL, 0x3feea47eb03a5585ULL,   \
    0x3feea09e667f3bcdULL, 0x3fee9f75e8ec5f74ULL, 0x3feea11473eb0187ULL, 0x3feea589994cce13ULL,   \
    0x3feeace5422aa0dbULL, 0x3feeb737b0cdc5e5ULL, 0x3feec49182a3f090ULL, 0x3feed503b23e255dULL,   \
    0x3feee89f995ad3adULL, 0x3feeff76f2fb5e47ULL, 0x3fef199bdd85529cULL, 0x3fef3720dcef9069ULL,   \
    0x3fef5818dcfba487ULL, 0x3fef7c97337b9b5fULL, 0x3fefa4afa2a490daULL, 0x3fefd0765b6e4540ULL
__device__ __constant__ unsigned long long jd_exp2f_tab[32] = {JD_EXP2F_TAB};
static const unsigned long long jd_exp2f_tab_host[32] = {JD_EXP2F_TAB};     // jd_debug_expf(device = -1)

// one source for the device function and its host twin (jd_debug_expf checks both against libm)
__host__ __device__ __forceinline__ float jd_expf_impl(float x, const unsigned long long *tab)
{
    const double InvLn2N = 0x1.71547652b82fep+0 * 32.0;
    const double SHIFT = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0;
    const double C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0;
    const double C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
    double z = InvLn2N * (double)x;
    double kd = z + SHIFT;
    unsigned long long ki;
    memcpy(&ki, &kd, sizeof ki);
    kd -= SHIFT;
    double r = z - kd;
    unsigned long long t = tab[ki & 31];
    t += ki << 47;
    double s;
    memcpy(&s, &t, sizeof s);
    double p = C0 * r + C1;
    double r2 = r * r;
    double y = C2 * r + 1.0;
    y = p * r2 + y;
    y = y * s;
    return (float)y;
}
__device__ __forceinline__ float jd_expf(float x) { return jd_expf_impl(x, jd_exp2f_tab); }

// glibc 2.35 log (sysdeps/ieee754/dbl-64/e_log.c, ARM optimized-routines algorithm) as the x86-64 libm runs it: the
// FMA build its ifunc selects, with the contractions GCC makes under -mfma written out as fma() here (this library builds
// with -ffp-contract=off).  __log_data: 128 (invc, logc) pairs, then ln2hi / ln2lo and the polynomials below.  Only
// what logAdd hands it is supported: y = 1 + e, e in (0, 1] - positive, normal, finite (no special cases).  Equal to
// the host libm for every float d in [-18.42, 0] (tests/test_logadd.py, through jd_debug_log1pe).
#define JD_LOG_TAB                                                                                          \
    0x3ff734f0c3e0de9fULL, 0xbfd7cc7f79e69000ULL, 0x3ff713786a2ce91fULL, 0xbfd76feec20d0000ULL,   \
    0x3ff6f26008fab5a0ULL, 0xbfd713e31351e000ULL, 0x3ff6d1a61f138c7dULL, 0xbfd6b85b38287800ULL,   \
    0x3ff6b1490bc5b4d1ULL, 0xbfd65d5590807800ULL, 0x3ff69147332f0cbaULL, 0xbfd602d076180000ULL,   \
    0x3ff6719f18224223ULL, 0xbfd5a8ca86909000ULL, 0x3ff6524f99a51ed9ULL, 0xbfd54f4356035000ULL,   \
    0x3ff63356aa8f24c4ULL, 0xbfd4f637c36b4000ULL, 0x3ff614b36b9ddc14ULL, 0xbfd49da7fda85000ULL,   \
    0x3ff5f66452c65c4cULL, 0xbfd445923989a800ULL, 0x3ff5d867b5912c4fULL, 0xbfd3edf439b0b800ULL,   \
    0x3ff5babccb5b90deULL, 0xbfd396ce448f7000ULL, 0x3ff59d61f2d91a78ULL, 0xbfd3401e17bda000ULL,   \
    0x3ff5805612465687ULL, 0xbfd2e9e2ef468000ULL, 0x3ff56397cee76bd3ULL, 0xbfd2941b3830e000ULL,   \
    0x3ff54725e2a77f93ULL, 0xbfd23ec58cda8800ULL, 0x3ff52aff42064583ULL, 0xbfd1e9e129279000ULL,   \
    0x3ff50f22dbb2bddfULL, 0xbfd1956d2b48f800ULL, 0x3ff4f38f4734ded7ULL, 0xbfd141679ab9f800ULL,   \
    0x3ff4d843cfde2840ULL, 0xbfd0edd094ef9800ULL, 0x3ff4bd3ec078a3c8ULL, 0xbfd09aa518db1000ULL,   \
    0x3ff4a27fc3e0258aULL, 0xbfd047e65263b800ULL, 0x3ff4880524d48434ULL, 0xbfcfeb224586f000ULL,   \
    0x3ff46dce1b192d0bULL, 0xbfcf474a7517b000ULL, 0x3ff453d9d3391854ULL, 0xbfcea4443d103000ULL,   \
    0x3ff43a2744b4845aULL, 0xbfce020d44e9b000ULL, 0x3ff420b54115f8fbULL, 0xbfcd60a22977f000ULL,   \
    0x3ff40782da3ef4b1ULL, 0xbfccc00104959000ULL, 0x3ff3ee8f5d57fe8fULL, 0xbfcc202956891000ULL,   \
    0x3ff3d5d9a00b4ce9ULL, 0xbfcb81178d811000ULL, 0x3ff3bd60c010c12bULL, 0xbfcae2c9ccd3d000ULL,   \
    0x3ff3a5242b75dab8ULL, 0xbfca45402e129000ULL, 0x3ff38d22cd9fd002ULL, 0xbfc9a877681df000ULL,   \
    0x3ff3755bc5847a1cULL, 0xbfc90c6d69483000ULL, 0x3ff35dce49ad36e2ULL, 0xbfc87120a645c000ULL,   \
    0x3ff34679984dd440ULL, 0xbfc7d68fb4143000ULL, 0x3ff32f5cceffcb24ULL, 0xbfc73cb83c627000ULL,   \
    0x3ff3187775a10d49ULL, 0xbfc6a39a9b376000ULL, 0x3ff301c8373e3990ULL, 0xbfc60b3154b7a000ULL,   \
    0x3ff2eb4ebb95f841ULL, 0xbfc5737d76243000ULL, 0x3ff2d50a0219a9d1ULL, 0xbfc4dc7b8fc23000ULL,   \
    0x3ff2bef9a8b7fd2aULL, 0xbfc4462c51d20000ULL, 0x3ff2a91c7a0c1babULL, 0xbfc3b08abc830000ULL,   \
    0x3ff293726014b530ULL, 0xbfc31b996b490000ULL, 0x3ff27dfa5757a1f5ULL, 0xbfc2875490a44000ULL,   \
    0x3ff268b39b1d3bbfULL, 0xbfc1f3b9f879a000ULL, 0x3ff2539d838ff5bdULL, 0xbfc160c8252ca000ULL,   \
    0x3ff23eb7aac9083bULL, 0xbfc0ce7f57f72000ULL, 0x3ff22a012ba940b6ULL, 0xbfc03cdc49fea000ULL,   \
    0x3ff2157996cc4132ULL, 0xbfbf57bdbc4b8000ULL, 0x3ff201201dd2fc9bULL, 0xbfbe370896404000ULL,   \
    0x3ff1ecf4494d480bULL, 0xbfbd17983ef94000ULL, 0x3ff1d8f5528f6569ULL, 0xbfbbf9674ed8a000ULL,   \
    0x3ff1c52311577e7cULL, 0xbfbadc79202f6000ULL, 0x3ff1b17c74cb26e9ULL, 0xbfb9c0c3e7288000ULL,   \
    0x3ff19e010c2c1ab6ULL, 0xbfb8a646b372c000ULL, 0x3ff18ab07bb670bdULL, 0xbfb78d01b3ac0000ULL,   \
    0x3ff1778a25efbcb6ULL, 0xbfb674f145380000ULL, 0x3ff1648d354c31daULL, 0xbfb55e0e6d878000ULL,   \
    0x3ff151b990275fddULL, 0xbfb4485cdea1e000ULL, 0x3ff13f0ea432d24cULL, 0xbfb333d94d6aa000ULL,   \
    0x3ff12c8b7210f9daULL, 0xbfb22079f8c56000ULL, 0x3ff11a3028ecb531ULL, 0xbfb10e4698622000ULL,   \
    0x3ff107fbda8434afULL, 0xbfaffa6c6ad20000ULL, 0x3ff0f5ee0f4e6bb3ULL, 0xbfadda8d4a774000ULL,   \
    0x3ff0e4065d2a9fceULL, 0xbfabbcece4850000ULL, 0x3ff0d244632ca521ULL, 0xbfa9a1894012c000ULL,   \
    0x3ff0c0a77ce2981aULL, 0xbfa788583302c000ULL, 0x3ff0af2f83c636d1ULL, 0xbfa5715e67d68000ULL,   \
    0x3ff09ddb98a01339ULL, 0xbfa35c8a49658000ULL, 0x3ff08cabaf52e7dfULL, 0xbfa149e364154000ULL,   \
    0x3ff07b9f2f4e28fbULL, 0xbf9e72c082eb8000ULL, 0x3ff06ab58c358f19ULL, 0xbf9a55f152528000ULL,   \
    0x3ff059eea5ecf92cULL, 0xbf963d62cf818000ULL, 0x3ff04949cdd12c90ULL, 0xbf9228fb8caa0000ULL,   \
    0x3ff038c6c6f0ada9ULL, 0xbf8c317b20f90000ULL, 0x3ff02865137932a9ULL, 0xbf8419355daa0000ULL,   \
    0x3ff0182427ea7348ULL, 0xbf781203c2ec0000ULL, 0x3ff008040614b195ULL, 0xbf60040979240000ULL,   \
    0x3fefe01ff726fa1aULL, 0x3f6feff384900000ULL, 0x3fefa11cc261ea74ULL, 0x3f87dc41353d0000ULL,   \
    0x3fef6310b081992eULL, 0x3f93cea3c4c28000ULL, 0x3fef25f63ceeadcdULL, 0x3f9b9fc114890000ULL,   \
    0x3feee9c8039113e7ULL, 0x3fa1b0d8ce110000ULL, 0x3feeae8078cbb1abULL, 0x3fa58a5bd001c000ULL,   \
    0x3fee741aa29d0c9bULL, 0x3fa95c8340d88000ULL, 0x3fee3a91830a99b5ULL, 0x3fad276aef578000ULL,   \
    0x3fee01e009609a56ULL, 0x3fb07598e598c000ULL, 0x3fedca01e577bb98ULL, 0x3fb253f5e30d2000ULL,   \
    0x3fed92f20b7c9103ULL, 0x3fb42edd8b380000ULL, 0x3fed5cac66fb5cceULL, 0x3fb606598757c000ULL,   \
    0x3fed272caa5ede9dULL, 0x3fb7da76356a0000ULL, 0x3fecf26e3e6b2ccdULL, 0x3fb9ab434e1c6000ULL,   \
    0x3fecbe6da2a77902ULL, 0x3fbb78c7bb0d6000ULL, 0x3fec8b266d37086dULL, 0x3fbd431332e72000ULL,   \
    0x3fec5894bd5d5804ULL, 0x3fbf0a3171de6000ULL, 0x3fec26b533bb9f8cULL, 0x3fc067152b914000ULL,   \
    0x3febf583eeece73fULL, 0x3fc147858292b000ULL, 0x3febc4fd75db96c1ULL, 0x3fc2266ecdca3000ULL,   \
    0x3feb951e0c864a28ULL, 0x3fc303d7a6c55000ULL, 0x3feb65e2c5ef3e2cULL, 0x3fc3dfc33c331000ULL,   \
    0x3feb374867c9888bULL, 0x3fc4ba366b7a8000ULL, 0x3feb094b211d304aULL, 0x3fc5933928d1f000ULL,   \
    0x3feadbe885f2ef7eULL, 0x3fc66acd2418f000ULL, 0x3feaaf1d31603da2ULL, 0x3fc740f8ec669000ULL,   \
    0x3fea82e63fd358a7ULL, 0x3fc815c0f51af000ULL, 0x3fea5740ef09738bULL, 0x3fc8e92954f68000ULL,   \
    0x3fea2c2a90ab4b27ULL, 0x3fc9bb3602f84000ULL, 0x3fea01a01393f2d1ULL, 0x3fca8bed1c2c0000ULL,   \
    0x3fe9d79f24db3c1bULL, 0x3fcb5b515c01d000ULL, 0x3fe9ae2505c7b190ULL, 0x3fcc2967ccbcc000ULL,   \
    0x3fe9852ef297ce2fULL, 0x3fccf635d5486000ULL, 0x3fe95cbaeea44b75ULL, 0x3fcdc1bd3446c000ULL,   \
    0x3fe934c69de74838ULL, 0x3fce8c01b8cfe000ULL, 0x3fe90d4f2f6752e6ULL, 0x3fcf5509c0179000ULL,   \
    0x3fe8e6528effd79dULL, 0x3fd00e6c121fb800ULL, 0x3fe8bfce9fcc007cULL, 0x3fd071b80e93d000ULL,   \
    0x3fe899c0dabec30eULL, 0x3fd0d46b9e867000ULL, 0x3fe87427aa2317fbULL, 0x3fd13687334bd000ULL,   \
    0x3fe84f00acb39a08ULL, 0x3fd1980d67234800ULL, 0x3fe82a49e8653e55ULL, 0x3fd1f8ffe0cc8000ULL,   \
    0x3fe8060195f40260ULL, 0x3fd2595fd7636800ULL, 0x3fe7e22563e0a329ULL, 0x3fd2b9300914a800ULL,   \
    0x3fe7beb377dcb5adULL, 0x3fd3187210436000ULL, 0x3fe79baa679725c2ULL, 0x3fd377266dec1800ULL,   \
    0x3fe77907f2170657ULL, 0x3fd3d54ffbaf3000ULL, 0x3fe756cadbd6130cULL, 0x3fd432eee32fe000ULL
__device__ __constant__ unsigned long long jd_log_tab[256] = {JD_LOG_TAB};
static const unsigned long long jd_log_tab_host[256] = {JD_LOG_TAB};     // jd_debug_log1pe / jd_debug_log_add (device = -1)

__host__ __device__ __forceinline__ double jd_u2d(unsigned long long u) { double d; memcpy(&d, &u, sizeof d); return d; }
__host__ __device__ __forceinline__ unsigned long long jd_d2u(double d) { unsigned long long u; memcpy(&u, &d, sizeof u); return u; }

__host__ __device__ inline double jd_log_libm_impl(double x, const unsigned long long *tab)
{
    const unsigned long long ix = jd_d2u(x);
    if (ix - 0x3fee000000000000ULL < 0x3ff1090000000000ULL - 0x3fee000000000000ULL) {   // [1 - 2^-4, 1 + 0x1.09p-4): poly1
        if (ix == 0x3ff0000000000000ULL) return 0.0;
        const double r = x - 1.0, r2 = r * r, r3 = r * r2;
        double p = __builtin_fma(r, -0x1.ffffffffffdcbp-3, 0x1.5555555555577p-2);
        p = __builtin_fma(r2, 0x1.999999995dd0cp-3, p);
        double q = __builtin_fma(r, 0x1.24924a344de30p-3, -0x1.55555556745a7p-3);
        q = __builtin_fma(r2, -0x1.fffffa4423d65p-4, q);
        double s = __builtin_fma(r, -0x1.999eb43b068ffp-4, 0x1.c7184282ad6cap-4);
        s = __builtin_fma(r2, 0x1.78182f7afd085p-4, s);
        s = __builtin_fma(r3, -0x1.5521375d145cdp-4, s);
        s = __builtin_fma(s, r3, q);
        s = __builtin_fma(s, r3, p);
        const double rhi = __builtin_fma(-r, 0x1p27, __builtin_fma(r, 0x1p27, r));     // r + w - w, w = r 2^27
        const double rlo = r - rhi;
        const double rr = rhi * rhi;
        const double hi = __builtin_fma(rr, -0.5, r);
        double lo = __builtin_fma(rr, -0.5, r - hi);
        lo = __builtin_fma(rlo * -0.5, r + rhi, lo);
        return hi + __builtin_fma(s, r3, lo);
    }
    // x = 2^k z, z in [0x1.6p-1, 0x1.6p+0); log x = k ln2 + log c + log1p(z / c - 1) for the c of z's subinterval
    const unsigned long long tmp = ix - 0x3fe6000000000000ULL;
    const int i = (int)((tmp >> 45) & 127);
    const double kd = (double)((long long)tmp >> 52);
    const double z = jd_u2d(ix - (tmp & (0xfffULL << 52)));
    const double invc = jd_u2d(tab[2 * i]), logc = jd_u2d(tab[2 * i + 1]);
    const double r = __builtin_fma(z, invc, -1.0);
    const double w = __builtin_fma(kd, 0x1.62e42fefa3800p-1, logc);                   // ln2hi
    const double hi = w + r;
    const double lo = __builtin_fma(kd, 0x1.ef35793c76730p-45, (w - hi) + r);         // ln2lo
    const double r2 = r * r;
    const double p = __builtin_fma(__builtin_fma(r, -0x1.55575e506c89fp-3, 0x1.999b324f10111p-3), r2,
                                   __builtin_fma(r, -0x1.fffffffeb4590p-3, 0x1.555555551305bp-2));
    return __builtin_fma(r * r2, p, __builtin_fma(r2, -0x1.0000000000001p-1, lo)) + hi;
}

// The fast value of log(1 + e), e in (0, 1], in double: a 129-entry table (c = 1 + k/128, invc = fl(1/c), logc = -log(invc),
// jd_fill_logtab) and log(y) = logc + log1p(y invc - 1) by a degree-7 polynomial.  Within 2 doubles of the libm's value for
// every float d in [-18.42, 0] (tests/test_logadd.py) but not equal to it: 39 M of those d differ by 1 or 2 ulp, and under
// cancellation (a logAdd result near 0) such a difference reaches the float.  jd_log_add_gate decides when it can.
struct JdLogTab { double invc, logc; };
static inline void jd_fill_logtab(JdLogTab *t)
{
    for (int k = 0; k <= 128; ++k) {
        const double c = 1.0 + k / 128.0;
        t[k].invc = (k == 0) ? 1.0 : 1.0 / c;
        t[k].logc = (k == 0) ? 0.0 : (double)(-logl((long double)t[k].invc));   // the identity holds for the ROUNDED invc
    }
}
__host__ __device__ __forceinline__ double jd_log1pe_table(double e, const JdLogTab *tab)
{
    const JdLogTab t = tab[(int)(e * 128.0 + 0.5)];
    const double r = __builtin_fma(1.0 + e, t.invc, -1.0);
    double q = 1.0 / 7.0;
    q = __builtin_fma(q, r, -1.0 / 6.0);
    q = __builtin_fma(q, r, 1.0 / 5.0);
    q = __builtin_fma(q, r, -1.0 / 4.0);
    q = __builtin_fma(q, r, 1.0 / 3.0);
    q = __builtin_fma(q, r, -1.0 / 2.0);
    q = __builtin_fma(q, r, 1.0);
    return t.logc + q * r;
}

// HTKFlatModels::logAdd (HTKFlatModels.cpp:266-293): a < c ? swap; d = y - x; d < -18.42 ? x : (float)(x + log(1.0 + expf(d))),
// log in double, as the host libm computes it.  Split in two so that jd_log_add2x2 can run two of them side by side:
//   gate    the table value m; rounding is monotone, so when x + (m - 2 ulp) and x + (m + 2 ulp) round to the same float the
//           libm's value, which lies between them, rounds to it too.  Returns whether they do not (the result is open).
//   settle  the cut and NaN (a NaN operand makes d NaN: expf and log propagate it in the reference).
// An open result takes jd_log_libm_impl (rare: the float result must lie within ~2 double ulps of a rounding boundary).
__host__ __device__ __forceinline__ bool jd_log_add_gate(float a, float c, const JdLogTab *tab, const unsigned long long *etab,
                                                         float &x, float &d, double &y, float &n)
{
    const bool s = a < c;
    x = s ? c : a;
    d = (s ? a : c) - x;
    // (the clamp keeps the table index in range for the steps whose result is discarded)
    const double e = (double)jd_expf_impl(fmaxf(d, -19.0f), etab);
    y = 1.0 + e;
    const unsigned long long m = jd_d2u(jd_log1pe_table(e, tab));                  // > 0
    n = (float)((double)x + jd_u2d(m - 2));
    return d >= -18.42 && n != (float)((double)x + jd_u2d(m + 2));
}
__host__ __device__ __forceinline__ float jd_log_add_settle(float x, float d, float n)
{
    return d < -18.42 ? x : (d != d ? d : n);                                       // HTKFlatModels.cpp:276 (double compare)
}
__host__ __device__ __forceinline__ float jd_log_add_impl(float a, float c, const JdLogTab *tab, const unsigned long long *etab,
                                                          const unsigned long long *ltab)
{
    float x, d, n;
    double y;
    if (jd_log_add_gate(a, c, tab, etab, x, d, y, n)) n = (float)((double)x + jd_log_libm_impl(y, ltab));
    return jd_log_add_settle(x, d, n);
}
// the generic kernel's (tab: the table of jd_fill_logtab in device memory)
__device__ __forceinline__ float jd_log_add(float a, float c, const JdLogTab *tab)
{
    return jd_log_add_impl(a, c, tab, jd_exp2f_tab, jd_log_tab);
}

// ------------------------------------------------------------------- GMM kernel

// par: [g][m][D][2] = (mean, ivar) interleaved; det: [g][m]; rows: row_src[r] is
// the frame index into feats (or -1); ll: [n_rows][G].
template <int DT>
__global__ __launch_bounds__(256) void jd_gmm_kernel(const float *__restrict__ feats,
                                                     const int *__restrict__ row_src, int n_rows,
                                                     const float *__restrict__ par,
                                                     const float *__restrict__ det,
                                                     const int *__restrict__ n_mix, int G, int M, int D,
                                                     float *__restrict__ ll, int skip_unused,
                                                     const JdLogTab *__restrict__ logtab)
{
    constexpr int DP = (DT > 0) ? (DT | 1) : 0;      // odd row stride: conflict-free per-lane rows
    extern __shared__ __align__(16) char smem[];
    const int dp = (DT > 0) ? DP : (D | 1);
    float *sx = (float *)smem;                        // [64][dp]
    float *so = sx + GMM_ROWS * dp;                   // [64][GMM_GT+1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Dn = (DT > 0) ? DT : D;
    // tiles = (64-row tile, GMM_GT-state group); the grid may be smaller than the number of
    // tiles (launch_gmm bounds how many wave slots the scoring may hold next to the search)
    const int n_rt = (n_rows + GMM_ROWS - 1) / GMM_ROWS, n_gt = (G + GMM_GT - 1) / GMM_GT;
    for (int tile = blockIdx.x; tile < n_rt * n_gt; tile += gridDim.x) {
    // row tile skewed by the state group: a bounded grid whose size is a multiple of n_rt would
    // otherwise hand each workgroup the same row tile every time (and the skipped ones no work)
    const int gt = tile / n_rt;
    const int r0 = ((tile + gt) % n_rt) * GMM_ROWS;
    const int g0 = gt * GMM_GT;
    // a tile whose rows are all unused (stream finished / chunk shorter than its slot) is skipped:
    // the valid rows of a stream's slot are a prefix of it and slots are multiples of the tile
    // (rows_per_slot % GMM_ROWS == 0), so the tile's first row decides
    if (skip_unused && row_src[r0] < 0) continue;
    __syncthreads();                                  // previous tile's LDS reads are done

    // stage the 64 x D feature tile (coalesced along D)
    for (int e = tid; e < GMM_ROWS * Dn; e += 256) {
        int r = e / Dn, j = e - r * Dn;
        int src = (r0 + r < n_rows) ? row_src[r0 + r] : -1;
        sx[r * dp + j] = (src >= 0) ? feats[(size_t)src * Dn + j] : 0.0f;
    }
    __syncthreads();

    float x[(DT > 0) ? DT : 1];
    if (DT > 0) {
#pragma unroll
        for (int j = 0; j < DT; ++j) x[j] = sx[lane * dp + j];
    }

    constexpr int GPW = GMM_GT / 4;                   // tied states per wave
    for (int gi = 0; gi < GPW; ++gi) {
        const int gl = wid * GPW + gi;                // wave-uniform
        const int g = g0 + gl;
        float acc = LZ;
        if (g < G) {
            const int nm = n_mix[g];
            const float *pg = par + (size_t)g * M * Dn * 2;
            const float *dg = det + (size_t)g * M;
            for (int m = 0; m < nm; ++m) {
                const float *pm = pg + (size_t)m * Dn * 2;
                float sum = 0.0f;
                if (DT > 0) {
#pragma unroll
                    for (int j = 0; j < DT; ++j) {
                        float xmu = x[j] - pm[2 * j];          // HTKFlatModels.cpp:249
                        sum += xmu * xmu * pm[2 * j + 1];      // :250  (no contraction)
                    }
                } else {
                    for (int j = 0; j < Dn; ++j) {
                        float xmu = sx[lane * dp + j] - pm[2 * j];
                        sum += xmu * xmu * pm[2 * j + 1];
                    }
                }
                float comp = (float)(-0.5 * (double)sum + (double)dg[m]);   // :254
                acc = jd_log_add(acc, comp, logtab);
            }
        }
        so[lane * (GMM_GT + 1) + gl] = acc;
    }
    __syncthreads();
    // coalesced store of the [64 rows][GMM_GT] tile
    for (int e = tid; e < GMM_ROWS * GMM_GT; e += 256) {
        int r = e / GMM_GT, c = e - r * GMM_GT;
        if (r0 + r < n_rows && g0 + c < G) ll[(size_t)(r0 + r) * G + g0 + c] = so[r * (GMM_GT + 1) + c];
    }
    }
}


// ---- the D = 39 kernel: TWO frames per lane, packed fp32 arithmetic.  GT tied states per tile (a quarter of them per
// wave): 64 for tables, 16 for the few rows of a streaming push - a tile is a chain of GT / 4 states x 16 mixtures per
// wave (0.3 ms at 64) whatever the number of rows, and a push of 64 frames is 47 such tiles on a chip of 1024 slots.
//
// A lane owns rows r and r + 64 of a 128-row tile; their vectors sit side by side in register
// pairs, so every VALU instruction of the distance loop is a packed one (v_pk_add_f32 /
// v_pk_mul_f32: two IEEE fp32 operations, no contraction - the same roundings as the reference's
// scalar code, HTKFlatModels.cpp:249-250) with the tied state's (mean, ivar) pairs arriving
// through the scalar cache.  logAdd (HTKFlatModels.cpp:266-293) evaluates log(1.0 + e), e in
// (0, 1], in double as the libm the reference links does: a table value, and where its last bits could
// move the float result the replica of glibc's log (jd_log_add_gate / jd_log_libm_impl above).
// (GMM_ROWS2 = 128, like the other tile constants: jd_score_plan.h)
typedef float jd_f2 __attribute__((ext_vector_type(2)));
// One logAdd step for the two frames of a lane, straight-line (no branch: some lane of a wave always takes the long path) and
// written pairwise so that the two dependent chains interleave.  etab is the LDS copy of jd_exp2f_tab, tab the LDS copy of
// the log table.  A result the table value leaves open (jd_log_add_gate) is NOT settled here: it becomes NaN, which every
// later step of the chain passes on, and jd_gmm_kernel39 scores a cell that ends NaN again with jd_log_add_impl once the
// tile's chains are done (its replica of the libm's log needs registers the distance loop holds).
__host__ __device__ __forceinline__ void jd_log_add2x2(float &a0, float &a1, float c0, float c1, const JdLogTab *tab,
                                                       const unsigned long long *etab)
{
    float x0, x1, d0, d1, n0, n1;
    double y0, y1;
    const bool o0 = jd_log_add_gate(a0, c0, tab, etab, x0, d0, y0, n0);
    const bool o1 = jd_log_add_gate(a1, c1, tab, etab, x1, d1, y1, n1);
    a0 = o0 ? __builtin_nanf("") : jd_log_add_settle(x0, d0, n0);
    a1 = o1 ? __builtin_nanf("") : jd_log_add_settle(x1, d1, n1);
}

// The cell (row r, tied state g) of jd_gmm_kernel39 again, one frame per lane with the exact logAdd throughout: the distance
// in the kernel's order and roundings (scalar IEEE operations equal the packed ones), features from memory (the tile's LDS
// copy is the output tile by then).
__device__ __noinline__ float jd_gmm_cell39(const float *__restrict__ feats, const int *__restrict__ row_src, int n_rows, int r,
                                            const float *__restrict__ pg, const float *__restrict__ dg, int nm,
                                            const JdLogTab *tab, const unsigned long long *etab)
{
    const int src = (r < n_rows) ? row_src[r] : -1;
    float acc = LZ;
    for (int m = 0; m < nm; ++m) {
        const float *pm = pg + (size_t)m * 39 * 2;
        float sum = 0.0f;
        for (int j = 0; j < 39; ++j) {
            const float u = ((src >= 0) ? feats[(size_t)src * 39 + j] : 0.0f) - pm[2 * j];
            const float z = u * u * pm[2 * j + 1];
            sum = (j == 0) ? z : sum + z;
        }
        const float c = (float)(-0.5 * (double)sum + (double)dg[m]);
        acc = (m == 0) ? (c <= LZ ? LZ : c) : jd_log_add_impl(acc, c, tab, etab, jd_log_tab);
    }
    return acc;
}

template <int GT>
__global__ __launch_bounds__(256, 4) void jd_gmm_kernel39(const float *__restrict__ feats,
                                                       const int *__restrict__ row_src, int n_rows,
                                                       const float *__restrict__ par,
                                                       const float *__restrict__ det,
                                                       const int *__restrict__ n_mix, int G, int M,
                                                       float *__restrict__ ll, int skip_unused,
                                                       const JdLogTab *__restrict__ logtab,
                                                       const int *__restrict__ rt_base, int n_rt_list)
{
    constexpr int DT = 39, DP = 39;                   // odd row stride: conflict-free per-lane rows
    extern __shared__ __align__(16) char smem[];
    JdLogTab *stab = (JdLogTab *)smem;                // [129] (+ pad)
    unsigned long long *setab = (unsigned long long *)(smem + 130 * sizeof(JdLogTab));   // [32]
    float *sx = (float *)(smem + 130 * sizeof(JdLogTab) + 32 * sizeof(unsigned long long));   // [128][DP]
    float *so = sx;                                   // [128][GT+1]: the feature tile is in registers by then
                                                      // (36 KB per workgroup: four of them share a CU's LDS)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 129; i += 256) stab[i] = logtab[i];
    if (tid < 32) setab[tid] = jd_exp2f_tab[tid];
    // rt_base (or null): the row tiles to score, by first row - the chunks of several streams, each in its own region of
    // the table (the resident kernel's side, jd_res_stage_many) - instead of every tile of rows [0, n_rows)
    const int n_rt = rt_base ? n_rt_list : (n_rows + GMM_ROWS2 - 1) / GMM_ROWS2, n_gt = (G + GT - 1) / GT;
    for (int tile = blockIdx.x; tile < n_rt * n_gt; tile += gridDim.x) {
        // row tile skewed by the state group (see jd_gmm_kernel)
        const int gt = tile / n_rt;
        const int r0 = rt_base ? rt_base[(tile + gt) % n_rt] : ((tile + gt) % n_rt) * GMM_ROWS2;
        const int g0 = gt * GT;
        if (skip_unused && row_src[r0] < 0) continue;
        __syncthreads();                              // previous tile's LDS reads are done
        for (int e = tid; e < GMM_ROWS2 * DT; e += 256) {
            const int r = e / DT, j = e - r * DT;
            const int src = (r0 + r < n_rows) ? row_src[r0 + r] : -1;
            sx[r * DP + j] = (src >= 0) ? feats[(size_t)src * DT + j] : 0.0f;
        }
        __syncthreads();
        jd_f2 x[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) { x[j].x = sx[lane * DP + j]; x[j].y = sx[(lane + 64) * DP + j]; }
        __syncthreads();                              // sx is re-used as the output tile
        constexpr int GPW = GT / 4;               // tied states per wave
        static_assert(GPW <= 16, "one bit per (state, frame) of a lane in open_cells");
        unsigned open_cells = 0;                  // bit gi: frame 0's cell of state gi is NaN (an open step, or NaN), bit 16 + gi: frame 1's
        for (int gi = 0; gi < GPW; ++gi) {
            const int gl = wid * GPW + gi;            // wave-uniform
            const int g = g0 + gl;
            float acc0 = LZ, acc1 = LZ;
            if (g < G) {
                const int nm = n_mix[g];
                const float *pg = par + (size_t)g * M * DT * 2;
                const float *dg = det + (size_t)g * M;
                for (int m = 0; m < nm; ++m) {
                    const float *pm = pg + (size_t)m * DT * 2;
                    jd_f2 sum = {0.0f, 0.0f};
                    // three dimensions at a time: their squared distances are independent, only the
                    // running sum is a chain (added in the reference's order)
#pragma unroll
                    for (int j = 0; j < DT; j += 3) {
                        const jd_f2 mu0 = {pm[2 * j], pm[2 * j]}, iv0 = {pm[2 * j + 1], pm[2 * j + 1]};
                        const jd_f2 mu1 = {pm[2 * j + 2], pm[2 * j + 2]}, iv1 = {pm[2 * j + 3], pm[2 * j + 3]};
                        const jd_f2 mu2 = {pm[2 * j + 4], pm[2 * j + 4]}, iv2 = {pm[2 * j + 5], pm[2 * j + 5]};
                        const jd_f2 u0 = x[j] - mu0, u1 = x[j + 1] - mu1, u2 = x[j + 2] - mu2;   // HTKFlatModels.cpp:249
                        const jd_f2 w0 = u0 * u0, w1 = u1 * u1, w2 = u2 * u2;
                        const jd_f2 z0 = w0 * iv0, z1 = w1 * iv1, z2 = w2 * iv2;                 // :250  (no contraction)
                        if (j == 0) sum = z0; else sum += z0;             // (0.0f + z0 == z0: z0 >= +0)
                        sum += z1; sum += z2;
                    }
                    const double dm = (double)dg[m];
                    const float c0 = (float)(-0.5 * (double)sum.x + dm), c1 = (float)(-0.5 * (double)sum.y + dm);   // :254
                    // logAdd(LOG_ZERO, c) is c for every c > LOG_ZERO, NaN for a NaN c and LOG_ZERO else (the difference is below
                    // -18.42, or the sum rounds back): the first mixture needs no exponential and no logarithm
                    if (m == 0) { acc0 = c0 <= LZ ? LZ : c0; acc1 = c1 <= LZ ? LZ : c1; }
                    else jd_log_add2x2(acc0, acc1, c0, c1, stab, setab);
                }
            }
            so[lane * (GT + 1) + gl] = acc0;
            so[(lane + 64) * (GT + 1) + gl] = acc1;
            open_cells |= (acc0 != acc0 ? 1u << gi : 0u) | (acc1 != acc1 ? 1u << (16 + gi) : 0u);
        }
        // the NaN cells again with the exact logAdd (their lanes' own entries of the output tile): the chains that met an open step
        // get their value, the NaN ones (a NaN feature or parameter) stay NaN
        for (unsigned o = open_cells; o; o &= o - 1) {
            const int b = __builtin_ctz(o), gl = wid * GPW + (b & 15), fr = b >> 4;
            const int g = g0 + gl;
            so[(lane + 64 * fr) * (GT + 1) + gl] = jd_gmm_cell39(feats, row_src, n_rows, r0 + lane + 64 * fr, par + (size_t)g * M * DT * 2,
                                                                det + (size_t)g * M, n_mix[g], stab, setab);
        }
        __syncthreads();
        for (int e = tid; e < GMM_ROWS2 * GT; e += 256) {
            const int r = e / GT, c = e - r * GT;
            if (r0 + r < n_rows && g0 + c < G) ll[(size_t)(r0 + r) * G + g0 + c] = so[r * (GT + 1) + c];
        }
    }
}


// ---- the D = 39 kernel with the scoring OPTION of jd_dec_set_scoring(JD_SCORE_FAST): the same tiling (two frames per lane, a quarter of a
// tile's tied states per wave, parameters through the scalar cache) without the reference's roundings.
//   distance   s = sqrt(ivar), t = -mean s (prepared on the host: AmDevBuf::par_fast): u = fma(x, s, t), sum = fma(u, u, sum) - two packed
//              fused multiply-adds per dimension and frame pair where the exact kernel issues four packed operations (sub, mul, mul, add)
//   logAdd     max + log(1 + exp(min - max)) in fp32 on the hardware's exp2 / log2 (v_exp_f32 / v_log_f32), the reference's -18.42 cut kept:
//              ~12 instructions per frame where the bit-exact replica (glibc's expf + an fp64 log(1 + e)) takes ~58
// north_star asks for path / acoustic scores within 1e-4 relative of the reference and identical words and times; this kernel is held to that
// (tests/test_gpu_fastscore.py: every fixture), not to bit equality - the DEFAULT stays jd_gmm_kernel39, whose table equals the CPU oracle's
// bit for bit.  Error: a log-likelihood of magnitude ~50-100 moves by ~1e-5 (39 fused terms of relative error 2^-24 each and one logAdd per
// mixture of absolute error ~1e-7).
__device__ __forceinline__ float jd_log_add_fast(float a, float c)
{
    const float x = fmaxf(a, c), y = fminf(a, c);
    const float d = y - x;
    const float e = __builtin_amdgcn_exp2f(d * 1.44269504088896340736f);      // exp(d), d <= 0
    const float l = __builtin_amdgcn_logf(1.0f + e) * 0.69314718055994530942f;
    return d < -18.42f ? x : x + l;                                           // HTKFlatModels.cpp:276 (LOG_ZERO - anything: -inf < cut)
}

template <int GT>
__global__ __launch_bounds__(256, 4) void jd_gmm_fast39(const float *__restrict__ feats, const int *__restrict__ row_src, int n_rows,
                                                      const float *__restrict__ par_fast, const float *__restrict__ det,
                                                      const int *__restrict__ n_mix, int G, int M, float *__restrict__ ll, int skip_unused,
                                                      const int *__restrict__ rt_base, int n_rt_list)
{
    constexpr int DT = 39, DP = 39;
    extern __shared__ __align__(16) char smem[];
    float *sx = (float *)smem;                        // [128][DP]
    float *so = sx;                                   // [128][GT+1]: the feature tile is in registers by then
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_rt = rt_base ? n_rt_list : (n_rows + GMM_ROWS2 - 1) / GMM_ROWS2, n_gt = (G + GT - 1) / GT;
    for (int tile = blockIdx.x; tile < n_rt * n_gt; tile += gridDim.x) {
        const int gt = tile / n_rt;                   // row tile skewed by the state group (see jd_gmm_kernel)
        const int r0 = rt_base ? rt_base[(tile + gt) % n_rt] : ((tile + gt) % n_rt) * GMM_ROWS2;
        const int g0 = gt * GT;
        if (skip_unused && row_src[r0] < 0) continue;
        __syncthreads();
        for (int e = tid; e < GMM_ROWS2 * DT; e += 256) {
            const int r = e / DT, j = e - r * DT;
            const int src = (r0 + r < n_rows) ? row_src[r0 + r] : -1;
            sx[r * DP + j] = (src >= 0) ? feats[(size_t)src * DT + j] : 0.0f;
        }
        __syncthreads();
        jd_f2 x[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) { x[j].x = sx[lane * DP + j]; x[j].y = sx[(lane + 64) * DP + j]; }
        __syncthreads();
        constexpr int GPW = GT / 4;
        for (int gi = 0; gi < GPW; ++gi) {
            const int gl = wid * GPW + gi;            // wave-uniform
            const int g = g0 + gl;
            float acc0 = LZ, acc1 = LZ;
            if (g < G) {
                const int nm = n_mix[g];
                const float *pg = par_fast + (size_t)g * M * DT * 2;
                const float *dg = det + (size_t)g * M;
                for (int m = 0; m < nm; ++m) {
                    const float *pm = pg + (size_t)m * DT * 2;
                    jd_f2 sum = {0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < DT; ++j) {
                        const jd_f2 sj = {pm[2 * j], pm[2 * j]}, tj = {pm[2 * j + 1], pm[2 * j + 1]};
                        const jd_f2 u = __builtin_elementwise_fma(x[j], sj, tj);
                        sum = __builtin_elementwise_fma(u, u, sum);
                    }
                    const float dm = dg[m];
                    const float c0 = __builtin_fmaf(-0.5f, sum.x, dm), c1 = __builtin_fmaf(-0.5f, sum.y, dm);
                    if (m == 0) { acc0 = LZ < c0 ? c0 : LZ; acc1 = LZ < c1 ? c1 : LZ; }
                    else { acc0 = jd_log_add_fast(acc0, c0); acc1 = jd_log_add_fast(acc1, c1); }
                }
            }
            so[lane * (GT + 1) + gl] = acc0;
            so[(lane + 64) * (GT + 1) + gl] = acc1;
        }
        __syncthreads();
        for (int e = tid; e < GMM_ROWS2 * GT; e += 256) {
            const int r = e / GT, c = e - r * GT;
            if (r0 + r < n_rows && g0 + c < G) ll[(size_t)(r0 + r) * G + g0 + c] = so[r * (GT + 1) + c];
        }
    }
}


// ---- JD_SCORE_FAST for every other vector size (D != 39): jd_gmm_fast39's arithmetic term for term - u = fma(x, s, t), sum = fma(u, u, sum)
// packed over a lane's frame pair, the dimensions in ascending order, c = fma(-0.5, sum, det), jd_log_add_fast over the mixtures - with D at
// run time.  The same 128-row tiles (rows r and r + 64 per lane), state groups of GT (a quarter per wave), row_src, skip_unused and tile list.
//   parameters  par_fast is [g][m][DP][2], DP = D rounded up to GMM_FAST_DC (upload_am_fast); the padding is s = t = 0 and the staged feature
//               tile is 0 there: u = 0 and sum = fma(0, 0, sum) = sum bit for bit.  A chunk of a mixture is 16 dwords through the scalar cache.
//   features    a slab of GMM_FAST_DS dimensions of the tile in LDS (33 KB: four workgroups share a CU), read a chunk of GMM_FAST_DC dimensions
//               at a time into registers (odd row stride: conflict-free) and used by up to GMM_FAST_MB mixtures of the wave's state, whose
//               running sums sit in registers.  D <= GMM_FAST_DS: the slab is the tile, staged once.  Above: the slabs are staged in turn
//               for every state and block of mixtures (the loops are then workgroup-uniform: bound by M, not n_mix) - 32 loads a lane
//               against 512 packed FMAs at 8 mixtures.
//   output      straight to the table (two dwords per lane and state): the LDS is the slab's, there is no room for a tile to transpose.
// (GMM_FAST_DC = 8, GMM_FAST_DS = 64: jd_score_plan.h)
#define GMM_FAST_MB 8               // (16: the compiler keeps scalar registers in vector lanes across the chunk loop)
template <int GT>
__global__ __launch_bounds__(256, 4) void jd_gmm_fast(const float *__restrict__ feats, const int *__restrict__ row_src, int n_rows,
                                                    const float *__restrict__ par_fast, const float *__restrict__ det,
                                                    const int *__restrict__ n_mix, int G, int M, int D, int DP, float *__restrict__ ll,
                                                    int skip_unused, const int *__restrict__ rt_base, int n_rt_list)
{
    constexpr int DC = GMM_FAST_DC, DS = GMM_FAST_DS, MB = GMM_FAST_MB, LS = DS + 1;
    extern __shared__ __align__(16) char smem[];
    float *sx = (float *)smem;                        // [128][LS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_slabs = (DP + DS - 1) / DS;
    const int n_rt = rt_base ? n_rt_list : (n_rows + GMM_ROWS2 - 1) / GMM_ROWS2, n_gt = (G + GT - 1) / GT;
    for (int tile = blockIdx.x; tile < n_rt * n_gt; tile += gridDim.x) {
        const int gt = tile / n_rt;                   // row tile skewed by the state group (see jd_gmm_kernel)
        const int r0 = rt_base ? rt_base[(tile + gt) % n_rt] : ((tile + gt) % n_rt) * GMM_ROWS2;
        const int g0 = gt * GT;
        if (skip_unused && row_src[r0] < 0) continue;
        // dimensions [slab DS, slab DS + w) of the tile's rows into sx (coalesced along the dimension; 0 for an unused row and the padding)
        auto stage = [&](int slab) {
            const int j0 = slab * DS, w = min(DS, DP - j0);
            __syncthreads();                          // the readers of what sx held are done
            for (int e = tid; e < GMM_ROWS2 * w; e += 256) {
                const int r = e / w, k = e - r * w;
                const int src = (r0 + r < n_rows) ? row_src[r0 + r] : -1;
                sx[r * LS + k] = (src >= 0 && j0 + k < D) ? feats[(size_t)src * D + j0 + k] : 0.0f;
            }
            __syncthreads();
        };
        if (n_slabs == 1) stage(0);
        const float *x0 = sx + lane * LS, *x1 = sx + (lane + 64) * LS;
        constexpr int GPW = GT / 4;
        for (int gi = 0; gi < GPW; ++gi) {
            const int g = g0 + wid * GPW + gi;        // wave-uniform
            const int nm = (g < G) ? n_mix[g] : 0;
            const float *pg = par_fast + (size_t)(g < G ? g : 0) * M * DP * 2;
            const float *dg = det + (size_t)(g < G ? g : 0) * M;
            float acc0 = LZ, acc1 = LZ;
            const int m_end = (n_slabs == 1) ? nm : M;    // (staging inside: every wave takes every turn)
            for (int m0 = 0; m0 < m_end; m0 += MB) {
                const int nb = min(MB, nm - m0);      // this wave's mixtures of the block (<= 0: none)
                jd_f2 sum[MB];
#pragma unroll
                for (int mi = 0; mi < MB; ++mi) sum[mi] = jd_f2{0.0f, 0.0f};
                for (int slab = 0; slab < n_slabs; ++slab) {
                    if (n_slabs > 1) stage(slab);
                    if (nb <= 0) continue;
                    const int j0 = slab * DS, w = min(DS, DP - j0);
                    for (int jc = 0; jc < w; jc += DC) {
                        jd_f2 x[DC];
#pragma unroll
                        for (int k = 0; k < DC; ++k) { x[k].x = x0[jc + k]; x[k].y = x1[jc + k]; }
                        // (one pointer for the chunk and a 32-bit stride between mixtures: a pointer per mixture kept over the loop costs
                        // more scalar registers than there are)
                        const float *pc = pg + ((size_t)m0 * DP + j0 + jc) * 2;
                        const unsigned ms = (unsigned)DP * 2u;
#pragma unroll
                        for (int mi = 0; mi < MB; ++mi) {
                            if (mi < nb) {
                                const float *pm = pc + (unsigned)mi * ms;
#pragma unroll
                                for (int k = 0; k < DC; ++k) {
                                    const jd_f2 sj = {pm[2 * k], pm[2 * k]}, tj = {pm[2 * k + 1], pm[2 * k + 1]};
                                    const jd_f2 u = __builtin_elementwise_fma(x[k], sj, tj);
                                    sum[mi] = __builtin_elementwise_fma(u, u, sum[mi]);
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (int mi = 0; mi < MB; ++mi) {
                    if (mi < nb) {
                        const float dm = dg[m0 + mi];
                        const float c0 = __builtin_fmaf(-0.5f, sum[mi].x, dm), c1 = __builtin_fmaf(-0.5f, sum[mi].y, dm);
                        if (m0 + mi == 0) { acc0 = LZ < c0 ? c0 : LZ; acc1 = LZ < c1 ? c1 : LZ; }
                        else { acc0 = jd_log_add_fast(acc0, c0); acc1 = jd_log_add_fast(acc1, c1); }
                    }
                }
            }
            if (g < G) {
                if (r0 + lane < n_rows) ll[(size_t)(r0 + lane) * G + g] = acc0;
                if (r0 + lane + 64 < n_rows) ll[(size_t)(r0 + lane + 64) * G + g] = acc1;
            }
        }
    }
}
