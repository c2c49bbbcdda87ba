// sr_grad_body.h — the body of the gradient kernels, included (as text, inside the kernel's braces) by
// sr_grad_impl.h: once with SR_GRAD_PARAM 0 for sr_grad_kernel(a), once with SR_GRAD_PARAM 1 for
// sr_grad_param_kernel(a, p), and once with SR_GRAD_LOSSX 1 for sr_grad_lossx_kernel(a, x).  A textual include and not a shared inlined function: the plain kernels
// then compile from exactly the text they always had (a force-inlined shared body moved their register
// counts; tools/kernel_resources.py compares them with the parent's).
// SR_GRAD_ROWOUT 1 (sr_grad_rows_kernel(a, d), sr_eval_grad_tree_array / sr_eval_diff_tree_array): the
// tangents are not scaled and summed but stored per row, and with d.feat the tangents are the features'
// (a feature operand x_f carries e_{f-1-k0}, a constant none) instead of the constants'.
#if SR_GRAD_ROWOUT
#define SR_GRAD_HOT_SRC 1  // basic_bin: the operand kinds that can carry a one-hot tangent (features too)
#else
#define SR_GRAD_HOT_SRC 2
#endif
  // rows per lane: lane + 64 j, j < R; a staged tile of TROWS rows is interpreted in TROWS / ROWS
  // sub-passes (round 5: one barrier pair and one staging round per 256 rows, not per 64 R; a lane
  // still meets its rows in row order, so the sums are the same bit for bit)
  constexpr int ROWS = 64 * R;                      // rows per program pass
  constexpr int TROWS = sr_grad_tile_rows(R);       // rows per staged tile
  constexpr int SUBS = TROWS / ROWS;
  static_assert(TROWS % ROWS == 0, "tile rows");
  constexpr int NV = 1 + KT;                 // value + tangents
  extern __shared__ __attribute__((aligned(16))) unsigned char sr_smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (uniform: item, k0 and jj live in SGPRs)
  const int lane = tid & 63;
  T* xs = reinterpret_cast<T*>(sr_smem);                       // [nf][TROWS]
  T* ys = xs + size_t(a.nf) * TROWS;                           // [TROWS]
  T* wsv = ys + TROWS;                                         // [TROWS] (weighted)
  T* stk = wsv + (a.w ? TROWS : 0);                            // [W][depth][NV][R][64]
  T* my_stk = stk + size_t(wave) * a.stack_depth * NV * R * 64 + lane;
#if SR_GRAD_PARAM
  // this wave's class bins (f64), behind the operand stacks: [KT][n_classes] filled by wave sums, or with
  // p.lane_slots > 0 (few slots x classes: sr_grad_param_lane_slots) one accumulator per lane,
  // [lane_slots][n_classes][64]: a lane adds its own rows in order, as the constants' acc does, and the 64
  // lanes are summed once per row block
  const int bins_per_wave = p.lane_slots > 0 ? p.lane_slots * p.n_classes * 64 : KT * p.n_classes;
  double* my_bins = reinterpret_cast<double*>(stk + size_t(W) * a.stack_depth * NV * R * 64) + size_t(wave) * bins_per_wave;
  for (int i = lane; i < bins_per_wave; i += 64) my_bins[i] = 0.0;
#endif

  int tg, rb, item, item_end = a.n_items;
  const int64_t* ridx = a.row_idx;  // GATHER: this block's row view
  if (a.segs == nullptr) {
    tg = int(blockIdx.x) % a.n_groups;
    rb = int(blockIdx.x) / a.n_groups;
    item = tg * W + wave;
  } else {
    // several row views in one launch (sr_eval_grad_batch_views): segment = one view's work items
    int lo = 0, hi = a.n_segs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.segs[mid].block0 <= int(blockIdx.x)) lo = mid;
      else hi = mid - 1;
    }
    const SrSegment sg = a.segs[lo];
    const int local = int(blockIdx.x) - sg.block0;
    tg = local % sg.groups;
    rb = local / sg.groups;
    item = sg.pos0 + tg * W + wave;
    item_end = sg.pos0 + sg.n_pos;
    ridx += sg.row_off;
  }
  const bool active = item < item_end;
  uint32_t pb = 0u, pe = 0u, k0 = 0u, cb = 0u, nconst = 0u;
#if SR_GRAD_PARAM
  uint32_t wpar = 0xffffffffu;
  int qp0 = 0, np = 0;
  const T* prow = nullptr;
#endif
  if (active) {
    const uint32_t t = a.item_tree[item];
    pb = a.offsets[t];
    pe = a.offsets[t + 1];
    k0 = a.item_k0[item];
    cb = a.const_off[t];
    nconst = a.const_off[t + 1] - cb;
#if SR_GRAD_PARAM
    {
      // the window's parameter tangents: positions qp0 .. qp0 + np - 1 (the constants come first), lane q
      // holds the parameter index of tangent k0 + q (none: all ones)
      const uint32_t ub = p.tan_off[t], nused = p.tan_off[t + 1] - ub;
      const uint32_t s = k0 + uint32_t(lane);
      if (lane < KT && s >= nconst && s - nconst < nused) wpar = p.tan_par[ub + (s - nconst)];
      qp0 = k0 < nconst ? int(nconst - k0) : 0;
      const int q1 = int(nconst + nused - k0) < KT ? int(nconst + nused - k0) : KT;
      np = q1 > qp0 ? q1 - qp0 : 0;
      prow = p.ptab + size_t(t) * size_t(p.p_stride);
    }
#endif
  }
  // this tree's constants: lane c holds constant c (programs are short: <= 64 constants per window
  // of lanes, more live in further registers of the same lane set)
  T cval0 = T(0), cval1 = T(0);
  if (active && uint32_t(lane) < nconst) cval0 = a.consts[cb + lane];
  if (active && uint32_t(lane) + 64u < nconst) cval1 = a.consts[cb + 64 + lane];

#if SR_GRAD_ROWOUT
  // where this item's tangents go and how many of the window's KT are the tree's; a non-finite tangent
  // of a valid row anywhere in the row block
  uint64_t out0 = 0;
  int nq = 0;
  if (active) {
    out0 = d.item_out[item];
    nq = int(d.item_nq[item]);
  }
  bool any_bad = false;
#else
  double acc[KT];  // per-lane f64 accumulators across the row block
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = 0.0;
#endif
  const bool weighted = a.w != nullptr;
  sr_libm_lds_fill(tid, W * 64);  // libm tables (visible after the first tile's barrier)

  for (int tile = 0; tile < a.tiles_per_block; ++tile) {
    const int64_t tile0 = (int64_t(rb) * a.tiles_per_block + tile) * TROWS;
    if (tile0 >= a.n_rows) break;
    __syncthreads();
    for (int i = tid; i < TROWS; i += W * 64) {
      const int64_t v = tile0 + i;
      const int64_t src = GATHER ? ridx[v < a.n_rows ? v : 0] : (v < a.n_rows ? v : 0);
      for (int f = 0; f < a.nf; ++f) xs[f * TROWS + i] = a.X[int64_t(f) * a.ld + src];
#if !SR_GRAD_ROWOUT
      ys[i] = a.y[src];
      if (weighted) wsv[i] = a.w[src];
#else
      (void)weighted;  // (no y, no weights: the tangents go out as they are)
#endif
    }
    __syncthreads();
    if (!active || pe == pb) continue;
    // the program's first window, kept across the sub-passes (programs are almost always <= 64)
    uint4 cw0 = make_uint4(0u, 0u, 0u, 0u);
    if (pb + lane < pe) cw0 = sr_load_window(a.code, pb + lane);
    for (int sub = 0; sub < SUBS; ++sub) {
    const int ro = sub * ROWS;  // the sub-pass's first row in the tile
    const int64_t row0 = tile0 + ro;
    if (row0 >= a.n_rows) break;

    T v[R];
    T dv[R][KT];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      v[j] = T(0);
#pragma unroll
      for (int q = 0; q < KT; ++q) dv[j][q] = T(0);
    }
    for (uint32_t base = pb; base < pe; base += 64u) {
      uint4 cw = cw0;
      if (base != pb) {
        cw = make_uint4(0u, 0u, 0u, 0u);
        if (base + lane < pe) cw = sr_load_window(a.code, base + lane);
      }
      const uint32_t n_here = __builtin_amdgcn_readfirstlane((pe - base < 64u) ? pe - base : 64u);
      for (uint32_t k = 0; k < n_here; ++k) {
        const uint32_t opc = uint32_t(__builtin_amdgcn_readlane(int(cw.x), int(k)));
        const uint32_t meta = uint32_t(__builtin_amdgcn_readlane(int(cw.y), int(k)));
        const uint32_t idx = meta & SR_M_INDEX;  // feature / stack slot / constant slot
        // a constant operand: its value (wave-uniform) and its one-hot tangent e_{idx-k0}
        auto const_val = [&]() __attribute__((always_inline)) -> T {
          return idx < 64u ? sr_readlane_val<T>(cval0, idx) : sr_readlane_val<T>(cval1, idx - 64u);
        };
#if SR_GRAD_ROWOUT
        // the leaf operand's own tangent slot: a constant's in constant mode, a feature's (LOAD_FEAT, the
        // F variants of the binaries) in feature mode, -1 for the other kind (its tangents are zero)
        const bool feat_operand = opc == SR_OP_LOAD_FEAT || opc == SR_OP_LOAD_FEAT_PUSH ||
                                  (opc >= SR_OP_BINARY0 && opc < SR_OP_LOAD_PARAM &&
                                   ((opc - SR_OP_BINARY0) % 6u == SR_V_FL || (opc - SR_OP_BINARY0) % 6u == SR_V_FR));
        const int jj = feat_operand == (d.feat != 0) ? int(idx) - int(k0) : -1;
#elif !SR_GRAD_PARAM
        const int jj = int(idx) - int(k0);
#else
        // (a parameter operand: its tangent's position in the window, -1: not a tangent of this window)
        int jj = int(idx) - int(k0);
        if (opc >= SR_OP_LOAD_PARAM && opc < SR_OP_PAIR0) {
          const uint64_t m = sr_ballot(wpar == idx);
          jj = m ? int(__builtin_ctzll(m)) : -1;
        }
        // row j's value of parameter idx, gathered by the row's class (the last staged row)
        auto param_val = [&](int j) __attribute__((always_inline)) -> T {
          return prow[size_t(idx) * size_t(p.n_classes) + size_t(int(xs[size_t(a.nf - 1) * TROWS + ro + j * 64 + lane]))];
        };
#endif
        const T* xrow = xs + size_t(idx) * TROWS + ro + lane;
        const T* sp = my_stk + size_t(idx) * NV * R * 64;
        auto push = [&]() __attribute__((always_inline)) {
          T* pp = my_stk + size_t(((meta >> SR_M_PUSH_SHIFT) & 0x3fu) - 1u) * NV * R * 64;
#pragma unroll
          for (int j = 0; j < R; ++j) {
            pp[j * 64] = v[j];
#pragma unroll
            for (int q = 0; q < KT; ++q) pp[((q + 1) * R + j) * 64] = dv[j][q];
          }
        };
        // r = op(a, b) and its tangents dr = pa da + pb db (pa, pb: the partials) for one of the
        // BASIC binaries with the operand variant known at compile time (round 5: one flat dispatch
        // per instruction instead of decoding the variant; the operand's tangent is known zero for a
        // feature and one-hot for a constant, so those products are not computed).  Every value is
        // the one the general form fma(pa, da, pb db) gives: a product by an exact 0 or 1 and a sum
        // with an exact 0 are exact (up to the sign of a zero, which the gradient sums cannot see),
        // and the skipped product by the zero tangent is still added as (partial x 0) — NaN when that
        // partial is not finite (a DIV by a tiny feature: r finite, -r / x overflows), as in the
        // general form.
        auto basic_bin = [&](auto op_c, auto var_c) __attribute__((always_inline)) {
          constexpr uint32_t B = decltype(op_c)::value;
          constexpr uint32_t V = decltype(var_c)::value;
          constexpr bool LEFT = V == SR_V_SL || V == SR_V_FL || V == SR_V_CL || V == SR_GV_PL;  // the operand is a
          // (SRC 3, PARAM builds: a parameter operand — a per-row value, one-hot at jj like a constant)
          constexpr int SRC = V >= SR_GV_PL ? 3 : ((V == SR_V_SL || V == SR_V_SR) ? 0 : ((V == SR_V_FL || V == SR_V_FR) ? 1 : 2));
          T cv = T(0);
          if constexpr (SRC == 2) cv = const_val();
          T fix[R] = {};  // constant operand: the tangent at its own slot jj, from the unscaled dv
          T d0[R] = {};
          const bool hot = SRC >= SR_GRAD_HOT_SRC && jj >= 0 && jj < KT;
          if (hot) {
#pragma unroll
            for (int q = 0; q < KT; ++q)
#pragma unroll
              for (int j = 0; j < R; ++j) d0[j] = q == jj ? dv[j][q] : d0[j];
          }
#pragma unroll
          for (int j = 0; j < R; ++j) {
#if SR_GRAD_PARAM
            const T ov = SRC == 3 ? param_val(j) : (SRC == 0 ? sp[j * 64] : (SRC == 1 ? xrow[j * 64] : cv));
#else
            const T ov = SRC == 0 ? sp[j * 64] : (SRC == 1 ? xrow[j * 64] : cv);
#endif
            const T av = LEFT ? ov : v[j], bv = LEFT ? v[j] : ov;
            const T rv = sr_binary<T>(B, av, bv);
            T pa, pbv;
            if constexpr (B == SR_B_DIV) {  // d/da = 1/b, d/db = -(a/b)/b = -r (1/b): one division fewer
              pa = T(1) / bv;
              pbv = -rv * pa;
            } else {
              sr_binary_partials<T>(B, av, bv, rv, &pa, &pbv);
            }
            v[j] = rv;
            if constexpr (SRC == 0) {  // stack operand: its tangents from the slot
#pragma unroll
              for (int q = 0; q < KT; ++q) {
                const T od = sp[((q + 1) * R + j) * 64];
                if constexpr (B == SR_B_ADD) {
                  dv[j][q] = LEFT ? od + dv[j][q] : dv[j][q] + od;
                } else if constexpr (B == SR_B_SUB) {
                  dv[j][q] = LEFT ? od - dv[j][q] : dv[j][q] - od;
                } else {
                  dv[j][q] = LEFT ? __builtin_fma(pa, od, pbv * dv[j][q]) : __builtin_fma(pa, dv[j][q], pbv * od);
                }
              }
            } else {
              // feature (zero tangent) or constant (one-hot at jj): every slot is the tos tangent
              // scaled by its own partial; a constant's own slot adds the constant's partial
              if (SRC >= SR_GRAD_HOT_SRC && hot) fix[j] = LEFT ? pa + pbv * d0[j] : __builtin_fma(pa, d0[j], pbv);
              if constexpr (B == SR_B_ADD) {
                // scale 1: unchanged
              } else if constexpr (B == SR_B_SUB) {
                if constexpr (LEFT) {
#pragma unroll
                  for (int q = 0; q < KT; ++q) dv[j][q] = -dv[j][q];
                }
              } else {
                const T sc = LEFT ? pbv : pa;
                const T z = (LEFT ? pa : pbv) * T(0);  // (the zero-tangent operand's product)
#pragma unroll
                for (int q = 0; q < KT; ++q) dv[j][q] = __builtin_fma(sc, dv[j][q], z);
              }
            }
          }
          if (SRC >= SR_GRAD_HOT_SRC && hot) {
#pragma unroll
            for (int q = 0; q < KT; ++q)
#pragma unroll
              for (int j = 0; j < R; ++j) dv[j][q] = q == jj ? fix[j] : dv[j][q];
          }
        };
#if SR_GRAD_PARAM
        {
          // the parametric opcodes (a block of its own: the plain build's switch stays as it was)
          if (opc >= SR_OP_LOAD_PARAM && opc < SR_OP_PAIR0) {
            switch (opc) {
              case SR_OP_LOAD_PARAM_PUSH:
                push();
                [[fallthrough]];
              case SR_OP_LOAD_PARAM:
#pragma unroll
                for (int j = 0; j < R; ++j) {
                  v[j] = param_val(j);
#pragma unroll
                  for (int q = 0; q < KT; ++q) dv[j][q] = q == jj ? T(1) : T(0);
                }
                break;
#define SR_GRAD_PCASE(B)                                                                                                              \
  case SR_PBIN_OPC(B, SR_V_PL): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_GV_PL>{}); break; \
  case SR_PBIN_OPC(B, SR_V_PR): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_GV_PR>{}); break;
              SR_GRAD_PCASE(SR_B_ADD)
              SR_GRAD_PCASE(SR_B_SUB)
              SR_GRAD_PCASE(SR_B_MUL)
              SR_GRAD_PCASE(SR_B_DIV)
#undef SR_GRAD_PCASE
              default: {
                // the other binaries with a parameter operand: the general tangent form
                const uint32_t b = (opc - SR_OP_PBIN0) / 2u + 1u;
                const bool left = (opc - SR_OP_PBIN0) % 2u == SR_V_PL;
                SrGVec<T, R> av, bv;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                  const T ov = param_val(j);
                  av[j] = left ? ov : v[j];
                  bv[j] = left ? v[j] : ov;
                }
                const SrGVec<T, R> rv = sr_grad_binary_val<T, R>(b, av, bv);
                const SrGVec<T, R> pa = sr_grad_binary_der<T, R, 0>(b, av, bv, rv);
                const SrGVec<T, R> pbv = sr_grad_binary_der<T, R, 1>(b, av, bv, rv);
#pragma unroll
                for (int j = 0; j < R; ++j) {
                  v[j] = rv[j];
#pragma unroll
                  for (int q = 0; q < KT; ++q) {
                    const T od = q == jj ? T(1) : T(0);
                    dv[j][q] = left ? __builtin_fma(pa[j], od, pbv[j] * dv[j][q]) : __builtin_fma(pa[j], dv[j][q], pbv[j] * od);
                  }
                }
                break;
              }
            }
            continue;
          }
        }
#endif
        switch (opc) {
          case SR_OP_LOAD_FEAT_PUSH:
            push();
            [[fallthrough]];
          case SR_OP_LOAD_FEAT:
#pragma unroll
            for (int j = 0; j < R; ++j) {
              v[j] = xrow[j * 64];
#pragma unroll
#if SR_GRAD_ROWOUT
              for (int q = 0; q < KT; ++q) dv[j][q] = q == jj ? T(1) : T(0);
#else
              for (int q = 0; q < KT; ++q) dv[j][q] = T(0);
#endif
            }
            break;
          case SR_OP_LOAD_CONST_PUSH:
            push();
            [[fallthrough]];
          case SR_OP_LOAD_CONST: {
            const T cv = const_val();
#pragma unroll
            for (int j = 0; j < R; ++j) {
              v[j] = cv;
#pragma unroll
              for (int q = 0; q < KT; ++q) dv[j][q] = q == jj ? T(1) : T(0);
            }
            break;
          }
#define SR_GRAD_BCASE(B)                                                                                  \
  case SR_BIN_OPC(B, SR_V_SL): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_V_SL>{}); break; \
  case SR_BIN_OPC(B, SR_V_SR): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_V_SR>{}); break; \
  case SR_BIN_OPC(B, SR_V_FL): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_V_FL>{}); break; \
  case SR_BIN_OPC(B, SR_V_FR): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_V_FR>{}); break; \
  case SR_BIN_OPC(B, SR_V_CL): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_V_CL>{}); break; \
  case SR_BIN_OPC(B, SR_V_CR): basic_bin(std::integral_constant<uint32_t, B>{}, std::integral_constant<uint32_t, SR_V_CR>{}); break;
          SR_GRAD_BCASE(SR_B_ADD)
          SR_GRAD_BCASE(SR_B_SUB)
          SR_GRAD_BCASE(SR_B_MUL)
          SR_GRAD_BCASE(SR_B_DIV)
#undef SR_GRAD_BCASE
          default:
            if (opc < SR_OP_BINARY0) {
              const uint32_t u = opc >= SR_OP_UNARY_INF0 ? opc - SR_OP_UNARY_INF0 : opc - SR_OP_UNARY0;
              // value and derivative rows: the BASIC operators with the loss kernel's own row bodies
              // (sr_unary_rows: the same values), the rest through the noinline row callees
              // (fused unaries: complete trees have finite inner values, so INFSUB never fires)
              T dfx[R];
              switch (u) {
                case SR_U_NEG:
#pragma unroll
                  for (int j = 0; j < R; ++j) {
                    v[j] = -v[j];
                    dfx[j] = T(-1);
                  }
                  break;
                case SR_U_SQUARE:
#pragma unroll
                  for (int j = 0; j < R; ++j) {
                    const T x = v[j];
                    v[j] = x * x;
                    dfx[j] = T(2) * x;
                  }
                  break;
                case SR_U_CUBE:
#pragma unroll
                  for (int j = 0; j < R; ++j) {
                    const T x = v[j];
                    v[j] = x * x * x;
                    dfx[j] = T(3) * x * x;
                  }
                  break;
                case SR_U_ABS:
#pragma unroll
                  for (int j = 0; j < R; ++j) {
                    const T x = v[j];
                    v[j] = sr_unary<T>(SR_U_ABS, x);
                    dfx[j] = sr_unary_deriv<T>(SR_U_ABS, x, v[j]);
                  }
                  break;
                case SR_U_SQRT:
#pragma unroll
                  for (int j = 0; j < R; ++j) {
                    v[j] = sr_unary<T>(SR_U_SQRT, v[j]);
                    dfx[j] = T(0.5) / v[j];
                  }
                  break;
                case SR_U_EXP:
                  sr_unary_rows<T, SR_U_EXP, R>(v);
#pragma unroll
                  for (int j = 0; j < R; ++j) dfx[j] = v[j];
                  break;
                case SR_U_LOG:
#pragma unroll
                  for (int j = 0; j < R; ++j) dfx[j] = T(1) / v[j];
                  sr_unary_rows<T, SR_U_LOG, R>(v);
                  break;
                case SR_U_COS:
#pragma unroll
                  for (int j = 0; j < R; ++j) dfx[j] = v[j];
                  sr_unary_rows<T, SR_U_COS, R>(v);
                  sr_unary_rows<T, SR_U_SIN, R>(dfx);
#pragma unroll
                  for (int j = 0; j < R; ++j) dfx[j] = -dfx[j];
                  break;
                case SR_U_SIN:
#pragma unroll
                  for (int j = 0; j < R; ++j) dfx[j] = v[j];
                  sr_unary_rows<T, SR_U_SIN, R>(v);
                  sr_unary_rows<T, SR_U_COS, R>(dfx);
                  break;
                default: {
                  SrGVec<T, R> x, y;
#pragma unroll
                  for (int j = 0; j < R; ++j) x[j] = v[j];
                  y = sr_grad_unary_val<T, R>(u, x);
                  x = sr_grad_unary_der<T, R>(u, x, y);
#pragma unroll
                  for (int j = 0; j < R; ++j) {
                    v[j] = y[j];
                    dfx[j] = x[j];
                  }
                  break;
                }
              }
#pragma unroll
              for (int j = 0; j < R; ++j) {
#pragma unroll
                for (int q = 0; q < KT; ++q) dv[j][q] = dfx[j] * dv[j][q];
              }
            } else {
              // the other binaries: value and partials through the row callees, the general tangent form
              const uint32_t b = (opc - SR_OP_BINARY0) / 6u + 1u;
              const uint32_t variant = (opc - SR_OP_BINARY0) % 6u;
              const bool left = variant == SR_V_SL || variant == SR_V_FL || variant == SR_V_CL;
              const bool from_feat = variant == SR_V_FL || variant == SR_V_FR;
              const bool from_stack = variant == SR_V_SL || variant == SR_V_SR;
              const T cv = (!from_feat && !from_stack) ? const_val() : T(0);
              auto operand = [&](int j, T& ov, T (&od)[KT]) {
                if (from_feat) {
                  ov = xrow[j * 64];
#pragma unroll
#if SR_GRAD_ROWOUT
                  for (int q = 0; q < KT; ++q) od[q] = q == jj ? T(1) : T(0);
#else
                  for (int q = 0; q < KT; ++q) od[q] = T(0);
#endif
                } else if (from_stack) {
                  ov = sp[j * 64];
#pragma unroll
                  for (int q = 0; q < KT; ++q) od[q] = sp[((q + 1) * R + j) * 64];
                } else {
                  ov = cv;
#pragma unroll
                  for (int q = 0; q < KT; ++q) od[q] = q == jj ? T(1) : T(0);
                }
              };
              auto tangents = [&](int j, T pa, T pbv, const T (&od)[KT]) {
                if (left) {
#pragma unroll
                  for (int q = 0; q < KT; ++q) dv[j][q] = __builtin_fma(pa, od[q], pbv * dv[j][q]);
                } else {
#pragma unroll
                  for (int q = 0; q < KT; ++q) dv[j][q] = __builtin_fma(pa, dv[j][q], pbv * od[q]);
                }
              };
              SrGVec<T, R> av, bv;
#pragma unroll
              for (int j = 0; j < R; ++j) {
                T ov, od[KT];
                operand(j, ov, od);
                av[j] = left ? ov : v[j];
                bv[j] = left ? v[j] : ov;
              }
              const SrGVec<T, R> rv = sr_grad_binary_val<T, R>(b, av, bv);
              const SrGVec<T, R> pa = sr_grad_binary_der<T, R, 0>(b, av, bv, rv);
              const SrGVec<T, R> pbv = sr_grad_binary_der<T, R, 1>(b, av, bv, rv);
#pragma unroll
              for (int j = 0; j < R; ++j) {
                T ov, od[KT];
                operand(j, ov, od);
                v[j] = rv[j];
                tangents(j, pa[j], pbv[j], od);
              }
            }
            break;
        }
      }
    }
#if SR_GRAD_ROWOUT
    // the tangents themselves, rows fastest: lane l of row group j stores row row0 + 64 j + l, so a
    // wave's store covers 64 consecutive elements; padded rows and the window's tangents past the tree's
    // are neither stored nor counted
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t row = row0 + j * 64 + lane;
      const bool valid = row < a.n_rows;
#pragma unroll
      for (int q = 0; q < KT; ++q) {
        if (q < nq && valid) {
          const T t = dv[j][q];
          d.out[out0 + uint64_t(q) * uint64_t(a.n_rows) + uint64_t(row)] = t;
          any_bad |= !sr_isfinite(t);
        }
      }
    }
#else
    // d loss / d constant: (d loss / d pred) * d pred / d constant, padded rows excluded
    T coefs[R];
#if SR_GRAD_LOSSX
    {
      // an expression loss: d value / d pred from the loss program, one pass over the lane's R rows; the
      // weight is the program's third argument (no coef *= w below)
      SrLxVec<T, R> pv, yv, wv;
#pragma unroll
      for (int j = 0; j < R; ++j) {
        pv[j] = v[j];
        yv[j] = ys[ro + j * 64 + lane];
        wv[j] = weighted ? wsv[ro + j * 64 + lane] : T(1);
      }
      pv = sr_lx_deriv<T, R, SrLxDevOps<T, R>>(lx.code, lx.n, pv, yv, wv);
#pragma unroll
      for (int j = 0; j < R; ++j) coefs[j] = pv[j];
    }
#else
    if (a.loss_kind == SR_LOSS_L2) {
#pragma unroll
      for (int j = 0; j < R; ++j) coefs[j] = sr_elem_loss_deriv<T>(SR_LOSS_L2, v[j], ys[ro + j * 64 + lane], T(0));
    } else {
      SrGVec<T, R> pv, yv;
#pragma unroll
      for (int j = 0; j < R; ++j) {
        pv[j] = v[j];
        yv[j] = ys[ro + j * 64 + lane];
      }
      pv = sr_grad_loss_der<T, R>(a.loss_kind, pv, yv, a.loss_param);
#pragma unroll
      for (int j = 0; j < R; ++j) coefs[j] = pv[j];
    }
#endif
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int r = j * 64 + lane;
      T coef = coefs[j];
#if !SR_GRAD_LOSSX
      if (weighted) coef *= wsv[ro + r];
#endif
      if (row0 + r >= a.n_rows) coef = T(0);
#pragma unroll
      for (int q = 0; q < KT; ++q) acc[q] = __builtin_fma(double(coef), double(dv[j][q]), acc[q]);
#if SR_GRAD_PARAM
      {
        // the parameter tangents of this 64-row group, binned by class (np, qp0 and every class picked
        // are wave-uniform); padded rows take no part
        // (acc[q] above also runs for the window's parameter slots: a few f64 FMAs nobody reads — the host
        //  takes those slots from the bins — kept so that the constants' code is the plain build's)
        if (np > 0 && p.lane_slots > 0) {
          const bool valid = row0 + r < a.n_rows;
          const int cls = int(xs[size_t(a.nf - 1) * TROWS + ro + r]);
          if (valid) {
#pragma unroll
            for (int q = 0; q < KT; ++q) {
              if (q < qp0 || q >= qp0 + np) continue;
              double* b = my_bins + (size_t(q - qp0) * p.n_classes + cls) * 64 + lane;
              *b = __builtin_fma(double(coef), double(dv[j][q]), *b);
            }
          }
        } else if (np > 0) {
          const bool valid = row0 + r < a.n_rows;
          const int cls = int(xs[size_t(a.nf - 1) * TROWS + ro + r]);
          uint64_t todo = sr_ballot(valid);
          while (todo) {
            const int c = __builtin_amdgcn_readlane(cls, int(__builtin_ctzll(todo)));
            const bool mine = valid && cls == c;
            todo &= ~sr_ballot(mine);
#pragma unroll
            for (int q = 0; q < KT; ++q) {
              if (q < qp0 || q >= qp0 + np) continue;
              const double s = sr_wave_sum<double>(mine ? double(coef) * double(dv[j][q]) : 0.0);
              if (lane == 0) my_bins[q * p.n_classes + c] += s;
            }
          }
        }
      }
#endif
    }
#endif  // !SR_GRAD_ROWOUT
    }  // sub-passes
  }
  if (!active) return;
#if SR_GRAD_ROWOUT
  {
    // one word per (row block, item): lane 0 writes whether any lane met a non-finite tangent
    const uint64_t m = sr_ballot(any_bad);
    if (lane == 0) d.bad[size_t(rb) * a.n_items + item] = m ? 1u : 0u;
  }
#else
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    const double s = sr_wave_sum<double>(acc[q]);
    if (lane == 0) a.part[(size_t(rb) * a.n_items + item) * KT + q] = s;
  }
#endif
#if SR_GRAD_PARAM
  {
    if (np > 0) {
      double* out = p.ppart + size_t(rb) * size_t(p.n_bins) + p.item_bin[item];
      // (the bins were written by this wave's own lanes — lane 0 in the wave-sum scheme — and a wave's LDS
      //  operations are ordered; the fence and wave barrier say so to the compiler)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (p.lane_slots > 0) {
        for (int i = 0; i < np * p.n_classes; ++i) {  // (wave-uniform trip count)
          const double s = sr_wave_sum<double>(my_bins[size_t(i) * 64 + lane]);
          if (lane == 0) out[i] = s;
        }
      } else {
        for (int i = lane; i < np * p.n_classes; i += 64) out[i] = my_bins[qp0 * p.n_classes + i];
      }
    }
  }
#endif
#undef SR_GRAD_HOT_SRC
