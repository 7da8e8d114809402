// The statements of the batched LSTM forward kernel (seq_lstm.hip's header comment describes the layout), included between the
// braces of a __global__ function of 512 threads with dynamic LDS of plan.lds_bytes that has in scope
//   template parameter / constant  bool VEC       rows of w_ih are read 128 bits at a time
//   constexpr bool TRAIN                         every step also stores the activated gates (i, f, g, o) and c_t
//   const Params p;  float* gates_out [B][T][4H], float* cell_out [B][T][H]  (read only where TRAIN)
// As text, not as a function: the inference kernel then compiles to the machine code it had before the training kernel existed.
    extern __shared__ float4 lds4[];
    float* const hs = reinterpret_cast<float*>(lds4);       // [2][16][HS]
    float* const xsb = hs + 2 * ROWS * HS;                  // [2][16][xs]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // (tells the compiler that it is uniform)
    const int r = lane & 15, g = lane >> 4;
    const int u0 = wave * 32;
    const long long b0 = (long long)blockIdx.x * ROWS;
    const int I = p.I, xs = p.xs, T = p.T;
    const int nci = (I + 15) / 16, nq = nci + HCHUNKS;
    const bool row_ok = b0 + r < p.B;

    // h_{-1} = 0, and the columns I .. 16 nci - 1 of both x tiles stay zero for the whole launch
    for (int e = tid; e < 2 * ROWS * (HS + xs); e += NT) hs[e] = 0.f;

    // x_t of the tile: wave w moves rows 2 w and 2 w + 1, a lane the columns lane + 64 j
    float xr[XR];
    auto load_x = [&](int t) {
#pragma unroll
        for (int j = 0; j < XR; ++j) {
            const int row = 2 * wave + j / (XR / 2), col = lane + 64 * (j % (XR / 2));
            const float* xrow = p.x + ((b0 + row) * T + t) * I;         // (uniform; dereferenced only for rows of the batch)
            xr[j] = (col < I && b0 + row < p.B) ? xrow[col] : 0.f;
        }
    };
    auto store_x = [&](int buf) {
#pragma unroll
        for (int j = 0; j < XR; ++j) {
            const int row = 2 * wave + j / (XR / 2), col = lane + 64 * (j % (XR / 2));
            if (col < I) xsb[(buf * ROWS + row) * xs + col] = xr[j];
        }
    };
    load_x(0);
    __syncthreads();
    store_x(0);

    // this lane's units: u0 + 16 ut + 4 g + reg
    float bias[2][4][4], c[2][4];
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            c[ut][reg] = 0.f;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) {
                const int n = gate * H + u0 + 16 * ut + 4 * g + reg;
                bias[ut][gate][reg] = p.b_ih[n] + p.b_hh[n];
            }
        }
    __syncthreads();

    // A fragments of K chunk q: chunks 0 .. nci - 1 walk w_ih, the rest w_hh.  A tile's first row is uniform, the lane adds
    // (its row, its k): one set of offsets per chunk for all eight tiles.  Past the end of a w_ih row (the tail of the last
    // chunk) a lane re-reads the row's last element(s) instead: the x tile holds zeros there, so the product adds nothing.
    const unsigned off_hh = (unsigned)(r * H + 4 * g);
    auto load_a = [&](int q, float4 (&a)[2][4]) {
        if (q < nci) {
            const int k0 = 16 * q + 4 * g;
            unsigned o[4];
            if constexpr (VEC) {
                o[0] = (unsigned)(r * I + min(k0, I - 4));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (unsigned)(r * I + min(k0 + j, I - 1));
            }
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int gate = 0; gate < 4; ++gate) {
                    const float* w = p.w_ih + (long long)(gate * H + u0 + 16 * ut) * I;
                    if constexpr (VEC) a[ut][gate] = *reinterpret_cast<const float4*>(w + o[0]);
                    else a[ut][gate] = make_float4(w[o[0]], w[o[1]], w[o[2]], w[o[3]]);
                }
        } else {
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int gate = 0; gate < 4; ++gate) {
                    const float* w = p.w_hh + ((gate * H + u0 + 16 * ut) * H + 16 * (q - nci));
                    a[ut][gate] = *reinterpret_cast<const float4*>(w + off_hh);
                }
        }
    };

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        if (t + 1 < T) load_x(t + 1);                                   // (lands under the products)
        f32x4 acc[2][4];
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) acc[ut][gate][reg] = bias[ut][gate][reg];
        const float* xb = xsb + (cur * ROWS + r) * xs + 4 * g;
        const float* hb = hs + (cur * ROWS + r) * HS + 4 * g;
        auto mma = [&](int q, const float4 (&a)[2][4]) {
            const float4 b = *reinterpret_cast<const float4*>(q < nci ? xb + 16 * q : hb + 16 * (q - nci));
            const float bm[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                    for (int gate = 0; gate < 4; ++gate) {
                        const float am = m == 0 ? a[ut][gate].x : m == 1 ? a[ut][gate].y : m == 2 ? a[ut][gate].z : a[ut][gate].w;
                        acc[ut][gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(am, bm[m], acc[ut][gate], 0, 0, 0);
                    }
        };
        // the fragments of chunk q + 1 are in flight while chunk q multiplies
        float4 a0[2][4], a1[2][4];
        load_a(0, a0);
        for (int q = 0; q < nq; q += 2) {
            if (q + 1 < nq) load_a(q + 1, a1);
            mma(q, a0);
            if (q + 1 < nq) {
                if (q + 2 < nq) load_a(q + 2, a0);
                mma(q + 1, a1);
            }
        }
        const bool write_out = row_ok && (!p.last_only || t + 1 == T);
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            float hv[4], act[TRAIN ? 4 : 1][4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float gi = apq::sigmoidf_(acc[ut][0][reg]), gf = apq::sigmoidf_(acc[ut][1][reg]);
                const float gg = apq::tanhf_(acc[ut][2][reg]), go = apq::sigmoidf_(acc[ut][3][reg]);
                c[ut][reg] = gf * c[ut][reg] + gi * gg;
                hv[reg] = go * apq::tanhf_(c[ut][reg]);
                if constexpr (TRAIN) {
                    act[0][reg] = gi; act[1][reg] = gf; act[2][reg] = gg; act[3][reg] = go;
                }
            }
            const int unit = u0 + 16 * ut + 4 * g;
            if constexpr (TRAIN) {
                if (row_ok) {
                    const long long bt = (b0 + r) * T + t;
#pragma unroll
                    for (int gate = 0; gate < 4; ++gate)
                        *reinterpret_cast<float4*>(gates_out + bt * (4 * H) + gate * H + unit) =
                            make_float4(act[gate][0], act[gate][1], act[gate][2], act[gate][3]);
                    *reinterpret_cast<float4*>(cell_out + bt * H + unit) = make_float4(c[ut][0], c[ut][1], c[ut][2], c[ut][3]);
                }
            }
            const float4 h4 = make_float4(hv[0], hv[1], hv[2], hv[3]);
            *reinterpret_cast<float4*>(hs + (nxt * ROWS + r) * HS + unit) = h4;
            if (write_out) {
                const long long row = p.last_only ? b0 + r : (b0 + r) * T + t;
                *reinterpret_cast<float4*>(p.out + row * H + unit) = h4;
            }
        }
        if (t + 1 < T) store_x(nxt);
        __syncthreads();            // h_t and x_{t+1} are complete; the tiles of step t may be overwritten in step t + 1
    }
