// The body of the one-pass selection of ONE row (trim_rows_sampled_kernel's algorithm), included textually by the two kernels that run it:
// trim_rows_sampled_kernel (a solo context's window) and fused_trim_select_kernel (the trimmed rows of a batch tick), so that there is
// one copy of the selection and the solo kernel compiles to the instructions it had as a kernel of its own (as a forced-inline function
// it did not: other operand orders and exec-mask sequences).  Included by kernels.hip inside a kernel that has declared
//   v (the row), n, k, samp_shift, margin, rt (kSqrt3 * the row's span), out_ub, out_lb, row (the output index), stat (optional),
//   tid, lane, wave, kWaves, kSelTag (trim_row_two_pass instantiation of the fallback) and the LDS arrays
//   buf (>= kWaves * kTrimSegCap words), h256[256], wsum / wcount[kWaves], s_pick[2], s_count, s_tot[4], red[2 * kWaves];
// it returns from the kernel.  Not a header: no include guard.
    const int nsamp = (n + (1 << samp_shift) - 1) >> samp_shift;
    const float* sv = v + trim_sample_offset(n);

    // (0) the sample: zeros counted, the rest into the level-0 histogram
    unsigned* hist = buf;
    for (int b = tid; b < kTrimBins; b += kTrimThreads) hist[b] = 0;
    __syncthreads();
    unsigned nzs = 0;
    for (int j = tid; j < nsamp; j += kTrimThreads) {
        const unsigned u = __float_as_uint(sv[j]);
        if (u == 0u) ++nzs; else atomicAdd(&hist[trim_bin0(u)], 1u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nzs += __shfl_xor(nzs, off, 64);
    if (lane == 0) wsum[wave] = nzs;
    __syncthreads();
    unsigned zeros_s = 0;
    for (int w = 0; w < kWaves; ++w) zeros_s += wsum[w];
    __syncthreads();
    const unsigned pos_s = (unsigned)nsamp - zeros_s;  // positive sample values
    unsigned a = 1u, bmax = 0xFFFFFFFFu;               // the bracket, inclusive, in bit patterns (a >= 1: zeros are never members)
    if (pos_s > 0u) {
        const long long r = ((long long)k * nsamp + n - 1) / n;  // the cut's expected rank in the sample
        long long lo_p = r - margin - (long long)zeros_s, hi_p = r + margin - (long long)zeros_s;
        if (hi_p < 1) hi_p = 1;
        unsigned bin, before;
        if (lo_p >= 1) {
            if (lo_p > (long long)pos_s) lo_p = pos_s;
            trim_pick(hist, (unsigned)lo_p, wsum, s_pick, bin, before);
            a = bin == 0 ? 1u : kTrimLo + (bin << 14);
        }
        if (hi_p <= (long long)pos_s) {
            trim_pick(hist, (unsigned)hi_p, wsum, s_pick, bin, before);
            if (bin != kTrimBins - 1) bmax = kTrimLo + ((bin + 1u) << 14) - 1u;
        }
    }
    __syncthreads();  // the histogram is dead: its LDS becomes the segments

    // (1) one pass over the row
    unsigned* seg = buf + wave * kTrimSegCap;
    unsigned nz = 0, nbelow = 0, wcnt = 0;  // wcnt: wave-uniform
    double acc[2] = {0.0, 0.0};
    auto below_a = [&](float x, unsigned u, bool valid) {
        const bool zero = valid && u == 0u, low = valid && u != 0u && u < a;
        nz += zero ? 1u : 0u;  // branch-free counters (as `if / else if` the compiler turned the two into a scratch array indexed by the case)
        nbelow += low ? 1u : 0u;
        if (low) {
            const float l = x - rt;
            acc[0] += (double)(x * x);
            acc[1] += (double)(l > 0.0f ? l * l : 0.0f);
        }
    };
    auto member = [&](unsigned u, bool in) {  // wave-level compaction in the order (call, lane)
        const unsigned long long m = __ballot(in);
        if (in) {
            const unsigned pos = wcnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (pos < (unsigned)kTrimSegCap) seg[pos] = u;
        }
        wcnt += (unsigned)__popcll(m);
    };
    auto visit4 = [&](const float4& p, bool valid) {
        const unsigned u0 = __float_as_uint(p.x), u1 = __float_as_uint(p.y), u2 = __float_as_uint(p.z), u3 = __float_as_uint(p.w);
        below_a(p.x, u0, valid); below_a(p.y, u1, valid); below_a(p.z, u2, valid); below_a(p.w, u3, valid);
        const bool i0 = valid && u0 >= a && u0 <= bmax, i1 = valid && u1 >= a && u1 <= bmax, i2 = valid && u2 >= a && u2 <= bmax, i3 = valid && u3 >= a && u3 <= bmax;
        if (__ballot(i0 | i1 | i2 | i3)) {  // rare: a few per cent of the row lie in the bracket
            member(u0, i0); member(u1, i1); member(u2, i2); member(u3, i3);
        }
    };
    {
        const int n4 = n >> 2;
        const float4* v4 = reinterpret_cast<const float4*>(v);
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = 0; base < n4; base += 4 * kTrimThreads) {  // every lane of a wave runs the same trips (the ballots need that)
            const int i0 = base + tid, i1 = i0 + kTrimThreads, i2 = i1 + kTrimThreads, i3 = i2 + kTrimThreads;
            const bool ok0 = i0 < n4, ok1 = i1 < n4, ok2 = i2 < n4, ok3 = i3 < n4;
            const float4 p0 = ok0 ? v4[i0] : zero4, p1 = ok1 ? v4[i1] : zero4, p2 = ok2 ? v4[i2] : zero4, p3 = ok3 ? v4[i3] : zero4;  // four 16-byte loads in flight per lane
            visit4(p0, ok0); visit4(p1, ok1); visit4(p2, ok2); visit4(p3, ok3);
        }
        const int t = (n4 << 2) + tid;
        if (wave == 0) {  // the row's last n % 4 elements
            const bool ok = t < n;
            const float x = ok ? v[t] : 0.f;
            const unsigned u = __float_as_uint(x);
            below_a(x, u, ok);
            member(u, ok && u >= a && u <= bmax);
        }
    }
    // totals
    unsigned t0 = nz, t1 = nbelow;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { t0 += __shfl_xor(t0, off, 64); t1 += __shfl_xor(t1, off, 64); }
    if (lane == 0) { wsum[wave] = t0; wcount[wave] = wcnt; h256[wave] = t1; }
    __syncthreads();
    if (tid == 0) {
        unsigned z = 0, c = 0, mem = 0, over = 0;
        for (int w = 0; w < kWaves; ++w) { z += wsum[w]; c += h256[w]; mem += wcount[w]; over |= wcount[w] > (unsigned)kTrimSegCap ? 1u : 0u; }
        s_tot[0] = z; s_tot[1] = c; s_tot[2] = mem; s_tot[3] = over;
    }
    __syncthreads();
    const unsigned zeros = s_tot[0], below = s_tot[0] + s_tot[1], members = s_tot[2], over = s_tot[3];
    const unsigned mycnt = wcount[wave] < (unsigned)kTrimSegCap ? wcount[wave] : (unsigned)kTrimSegCap;
    __syncthreads();
    if ((unsigned)k <= zeros) {  // the k smallest terms are all zero
        if (tid == 0) { out_ub[row] = 0.0f; out_lb[row] = 0.0f; if (stat) atomicAdd(&stat[0], 1ull); }
        return;
    }
    // (2) the exact check of the bracket
    if (over || (unsigned)k <= below || (unsigned)k - below > members) {
        if (tid == 0 && stat) { atomicAdd(&stat[0], 1ull); atomicAdd(&stat[1], 1ull); }
        trim_row_two_pass<kTrimFallbackCap, kSelTag>(v, n, k, rt, buf, buf + kTrimBins, wsum, s_pick, &s_count, red, out_ub, out_lb, row);
        return;
    }
    if (tid == 0 && stat) { atomicAdd(&stat[0], 1ull); atomicAdd(&stat[2], (unsigned long long)members); }
    // (3) the need-th smallest member: radix select on w = u - a, 8 bits per round
    unsigned need = (unsigned)k - below;  // 1 <= need <= members
    const unsigned width = bmax - a;      // w in [0, width]
    int nbits = 32 - __clz(width | 1u);
    int shift = ((nbits + 7) / 8) * 8 - 8;
    unsigned prefix = 0;                  // the bits of the answer above shift + 8
    for (; shift >= 0; shift -= 8) {
        if (tid < 256) h256[tid] = 0;
        __syncthreads();
        for (unsigned j = lane; j < mycnt; j += 64) {
            const unsigned w = seg[j] - a;
            if (shift + 8 >= 32 || (w >> (shift + 8)) == prefix) atomicAdd(&h256[(w >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned mine = 0, incl = 0;
        if (tid < 256) {  // waves 0..3: which digit holds rank `need`
            mine = h256[tid];
            incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned u = __shfl_up(incl, off, 64);
                if (lane >= off) incl += u;
            }
            if (lane == 63) wsum[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            unsigned base = 0;
            for (int w = 0; w < wave; ++w) base += wsum[w];
            const unsigned excl = base + incl - mine;
            if (excl < need && need <= excl + mine) { s_pick[0] = (unsigned)tid; s_pick[1] = excl; }  // exactly one thread
        }
        __syncthreads();
        prefix = (prefix << 8) | s_pick[0];
        need -= s_pick[1];
        __syncthreads();
    }
    const unsigned wk = prefix;  // w of the need-th smallest member; `need` is now its rank among its copies: that many copies count
    for (unsigned j = lane; j < mycnt; j += 64) {
        const unsigned u = seg[j];
        if (u - a < wk) {
            const float x = __uint_as_float(u);
            const float l = x - rt;
            acc[0] += (double)(x * x);
            acc[1] += (double)(l > 0.0f ? l * l : 0.0f);
        }
    }
    const double r = block_sum<2, kWaves>(acc, red);
    if (tid < 2) {
        const float x = __uint_as_float(a + wk);
        const float l = x - rt;
        const double extra = (double)need * (double)(tid == 0 ? x * x : (l > 0.0f ? l * l : 0.0f));
        (tid == 0 ? out_ub : out_lb)[row] = (float)(r + extra);
    }
