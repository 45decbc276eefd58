// linearize_pull.inc -- the body of k_linearize and of k_linearize_lm (kernels.hip.h includes it inside each of the two kernels,
// behind `constexpr bool LM`; TO, T, RK, D, PR and the argument `a` are the kernel's).  Every LM path is behind `if constexpr (LM)`
// and every such statement keeps the LM = false text in its else branch, so k_linearize compiles what it always did.
// k_linearize_br includes it too, behind `constexpr bool BR` (D = 3: a 2-D graph with bearing-only / range-only edges), by the same rule.
  using V4 = typename VecT<T>::V4;
  constexpr int NV = D / 3;             // V4s per node and per measurement
  constexpr int NT = D * (D + 1) / 2;   // lower triangle of the diagonal block, row-major: (0,0),(1,0),(1,1),...
  __shared__ double red[LIN_THREADS / 64];
  const int gid = blockIdx.x * LIN_THREADS + threadIdx.x;
  for (int i = gid; i < a.n_zero_words; i += gridDim.x * LIN_THREADS) a.zero_words[i] = 0u;
  for (int i = gid; i < a.n_fill_words; i += gridDim.x * LIN_THREADS) a.fill_words[i] = X_PENDING_WORD;
  opt_reset_in_first_thread(a);
  const LinPre lin_pre = opt_publish_preload(a);
  const T lambda = a.lambda_from_ctrl ? (T)a.ctrl->lambda : a.lambda;
  const int slot = gid / LIN_GROUP, sub = gid % LIN_GROUP;
  const int node = listed_node(a, slot);
  double chi = 0.0;
  T hd[NT], bv[D];
#pragma unroll
  for (int t = 0; t < NT; t++) hd[t] = 0;
#pragma unroll
  for (int t = 0; t < D; t++) bv[t] = 0;
  int nd = D;
  bool fx_self = false;   // rr_pgo_set_fixed: this group's node is held constant
  if (node >= 0) {
    if constexpr (D == 3 || LM) nd = a.node_dim[node];
    fx_self = a.fixed && a.fixed[node];
    V4 self[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) self[v] = a.pose[NV * node + v];
    const int q1 = a.inc_ptr[node + 1];
    for (int q = a.inc_ptr[node] + sub; q < q1; q += LIN_GROUP) {
      const int2 inc = a.inc_list[q];
      const int ent = inc.x;
      const bool fx_other = a.fixed && a.fixed[inc.y];   // rr_pgo_set_fixed: requested with the far pose, used behind the stores
      // sharded runs: an edge contributes to diagonal blocks, right-hand side and chi2 on ONE rank (bit 2, its
      // owner -- the other ranks' copies of a far endpoint are stale); the off-diagonal block of an edge between
      // two shared nodes is written by every rank (bit 3)
      if (!(ent & 12)) continue;
      const bool owns = ent & 4;
      const int k = ent >> 4, role = ent & 1;
      // ---- per dimension: the operands, e and J = the Jacobian of this endpoint (A in the from role, B in the to role)
      T W[D][D], e[D], J[D][D];
      [[maybe_unused]] EdgeRec<T> rec;                                 // SE(2)
      [[maybe_unused]] T B2[3][3];                                     // SE(2): B comes with A
      [[maybe_unused]] T ts[3], qs[4], to[3], qo[4], tz[3], qz[4];     // SE(3): B is evaluated where it is needed
      if constexpr (D == 3) {
        rec = a.e_rec[k];
        const V4 other = a.pose[inc.y];
        info_2d<T>(rec, W);
        T A[3][3];
        if constexpr (BR) {   // a bearing or range edge: a landmark edge whose measurement holds its kind in lane 3 (SE2_XY: 0)
          if (((ent >> 1) & 1) && rec.meas.w != (T)0) edge_linearize_2d_br<T>(role ? other : self[0], role ? self[0] : other, rec.meas, e, A, B2);
          else edge_linearize_2d<T>((ent >> 1) & 1, role ? other : self[0], role ? self[0] : other, rec.meas, e, A, B2);
        } else
        edge_linearize_2d<T>((ent >> 1) & 1, role ? other : self[0], role ? self[0] : other, rec.meas, e, A, B2);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int c = 0; c < 3; c++) J[r][c] = role ? B2[r][c] : A[r][c];
      } else {
        pose_3d<T>(self[0], self[1], ts, qs);
        pose_3d<T>(a.pose[2 * inc.y], a.pose[2 * inc.y + 1], to, qo);
        pose_3d<T>(a.e_meas[2 * k], a.e_meas[2 * k + 1], tz, qz);
        info_3d<T>(a.e_info + (int64_t)k * 21, W);
        if constexpr (LM) {
          if ((ent >> 1) & 1) {   // SE3_XYZ: the pose is the from node, the landmark the to node
            if (role) edge_linearize_3d_point<T>(1, to, qo, ts, tz, e, J);
            else edge_linearize_3d_point<T>(0, ts, qs, to, tz, e, J);
          } else {
            if (role) edge_linearize_3d<T>(1, to, qo, ts, qs, tz, qz, e, J);
            else edge_linearize_3d<T>(0, ts, qs, to, qo, tz, qz, e, J);
          }
        } else {
          if (role) edge_linearize_3d<T>(1, to, qo, ts, qs, tz, qz, e, J);
          else edge_linearize_3d<T>(0, ts, qs, to, qo, tz, qz, e, J);
        }
      }
      // ---- the frame
      T s_rob = 0;
      bool rob = false;
      if constexpr (RK != ROBUST_NONE) {
        s_rob = edge_chi2<D, T>(W, e);
        rob = !a.robust_mask || a.robust_mask[k];
        if (rob) {   // masked-off edges keep W as it is
          const T w = robust_weight<RK, T>(s_rob, a.robust_delta, a.robust_delta2, a.tls_lo, a.tls_hi, a.tls_cs, a.tls_mu);
#pragma unroll
          for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j < D; j++) W[i][j] *= w;
        }
      }
      T JW[D][D];   // J^T W
#pragma unroll
      for (int i = 0; i < D; i++)
#pragma unroll
        for (int j = 0; j < D; j++) {
          T s = 0;
#pragma unroll
          for (int r = 0; r < D; r++) s += J[r][i] * W[r][j];
          JW[i][j] = s;
        }
      if (a.write_system && owns) {
        int t = 0;
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
          for (int j = 0; j <= i; j++) {
            T s = 0;
#pragma unroll
            for (int r = 0; r < D; r++) s += JW[i][r] * J[r][j];
            hd[t++] += s;
          }
#pragma unroll
        for (int i = 0; i < D; i++) bv[i] += row_dot<D, T>(JW[i], e, 1);
      }
      if (role == 0) {
        // chi2 term e^T W e (:555,568), accumulated in f64; rho(e^T W e) under a robust kernel
        if constexpr (RK == ROBUST_NONE) {
          if (owns) chi += (double)edge_chi2<D, T>(W, e);   // every edge's term is owned by one rank
        } else {
          if (owns) chi += (double)(rob ? robust_rho<RK, T>(s_rob, a.robust_delta, a.robust_delta2, a.tls_lo, a.tls_hi, a.tls_cs, a.tls_mu) : s_rob);
        }
        if (a.write_system && (ent & 8)) {
          // ---- per dimension: the off-diagonal block H[from rows, to cols] = A^T W B and where it goes
          if constexpr (D == 3) {
            const int64_t so = rec.slot;
            TO *dst = a.hvals + (so >> 1);
            const bool tr = so & 1;
            const int d2 = ((ent >> 1) & 1) ? 2 : 3;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
              for (int j = 0; j < 3; j++) {
                if (j >= d2) continue;
                dst[tr ? j * 3 + i : i * d2 + j] = (TO)row_dot<3, T>(JW[i], &B2[0][j], 3);
              }
          } else {
            T e2[6], Bm[6][6];
            if constexpr (LM) {
              const bool point = (ent >> 1) & 1;
              if (point) edge_linearize_3d_point<T>(1, ts, qs, to, tz, e2, Bm);
              else edge_linearize_3d<T>(1, ts, qs, to, qo, tz, qz, e2, Bm);
              const int64_t so = a.e_slot[k];
              TO *dst = a.hvals + (so >> 1);
              const bool tr = so & 1;
              const int d2 = point ? 3 : 6;   // 6 x 3 into a landmark: the D == 3 rule with 6 and 3
#pragma unroll
              for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) {
                  if (j >= d2) continue;
                  dst[tr ? j * 6 + i : i * d2 + j] = (TO)row_dot<6, T>(JW[i], &Bm[0][j], 6);
                }
            } else {
            edge_linearize_3d<T>(1, ts, qs, to, qo, tz, qz, e2, Bm);
            const int64_t so = a.e_slot[k];
            TO *dst = a.hvals + (so >> 1);
            const bool tr = so & 1;
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
              for (int j = 0; j < 6; j++) dst[tr ? j * 6 + i : i * 6 + j] = (TO)row_dot<6, T>(JW[i], &Bm[0][j], 6);
            }
          }
          // rr_pgo_set_fixed: the block of an edge with a fixed endpoint (this node, or the other one) is overwritten with
          // zeros -- a second store of the same lane, behind everything the loop does otherwise
          if (fx_self | fx_other) {
            if constexpr (D == 3) {
              TO *dst = a.hvals + (rec.slot >> 1);
              const int cnt = ((ent >> 1) & 1) ? 6 : 9;   // 3 x 2 (landmark) or 3 x 3
#pragma unroll
              for (int t = 0; t < 9; t++)
                if (t < cnt) dst[t] = (TO)0;
            } else {
              TO *dst = a.hvals + (a.e_slot[k] >> 1);
              if constexpr (LM) {
                const int cnt = ((ent >> 1) & 1) ? 18 : 36;   // 6 x 3 (landmark) or 6 x 6
#pragma unroll
                for (int t = 0; t < 36; t++)
                  if (t < cnt) dst[t] = (TO)0;
              } else {
#pragma unroll
              for (int t = 0; t < 36; t++) dst[t] = (TO)0;
              }
            }
          }
        }
      }
    }
    if constexpr (PR) {
      const int p1 = a.prior_ptr[node + 1];
      for (int p = a.prior_ptr[node] + sub; p < p1; p += LIN_GROUP) {
        T W[D][D], e[D], J[D][D];
        // ---- per dimension: the operands, e and J = B of the edge identity -> node
        if constexpr (D == 3) {
          const EdgeRec<T> rec = a.prior_rec[p];
          info_2d<T>(rec, W);
          prior_linearize_2d<T>(nd == 2 ? 1 : 0, self[0], rec.meas, e, J);
        } else {
          T ts[3], qs[4], tz[3], qz[4];
          pose_3d<T>(self[0], self[1], ts, qs);
          pose_3d<T>(a.prior_meas[2 * p], a.prior_meas[2 * p + 1], tz, qz);
          info_3d<T>(a.prior_info + (int64_t)p * 21, W);
          if constexpr (LM) {
            if (nd == 3) prior_linearize_3d_point<T>(ts, tz, e, J);
            else prior_linearize_3d<T>(ts, qs, tz, qz, e, J);
          } else {
          prior_linearize_3d<T>(ts, qs, tz, qz, e, J);
          }
        }
        // ---- the frame, as for an edge in its `to` role
        T s_rob = 0;
        bool rob = false;
        if constexpr (RK != ROBUST_NONE) {
          s_rob = edge_chi2<D, T>(W, e);
          rob = a.prior_robust[p] != 0;
          if (rob) {
            const T w = robust_weight<RK, T>(s_rob, a.robust_delta, a.robust_delta2, a.tls_lo, a.tls_hi, a.tls_cs, a.tls_mu);
#pragma unroll
            for (int i = 0; i < D; i++)
#pragma unroll
              for (int j = 0; j < D; j++) W[i][j] *= w;
          }
        }
        if (a.write_system) {
          T JW[D][D];   // J^T W
#pragma unroll
          for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j < D; j++) {
              T s = 0;
#pragma unroll
              for (int r = 0; r < D; r++) s += J[r][i] * W[r][j];
              JW[i][j] = s;
            }
          int t = 0;
#pragma unroll
          for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
              T s = 0;
#pragma unroll
              for (int r = 0; r < D; r++) s += JW[i][r] * J[r][j];
              hd[t++] += s;
            }
#pragma unroll
          for (int i = 0; i < D; i++) bv[i] += row_dot<D, T>(JW[i], e, 1);
        }
        if constexpr (RK == ROBUST_NONE) chi += (double)edge_chi2<D, T>(W, e);
        else chi += (double)(rob ? robust_rho<RK, T>(s_rob, a.robust_delta, a.robust_delta2, a.tls_lo, a.tls_hi, a.tls_cs, a.tls_mu) : s_rob);
      }
    }
  }
  if (a.write_system) {
#pragma unroll
    for (int t = 0; t < NT; t++) hd[t] = group_sum8(hd[t]);
#pragma unroll
    for (int t = 0; t < D; t++) bv[t] = group_sum8(bv[t]);
    if (node >= 0 && sub == 0) {
      T add = lambda;
      if (node == a.anchor) add += (T)10000000.0;
      if (a.adds_diag && !a.adds_diag[node]) add = 0;
      // ---- per dimension: the diagonal block's layout
      TO *d = a.hvals + a.diag_off[node];
      if constexpr (D == 3) {
        if (nd == 3) {
          d[0] = (TO)(hd[0] + add); d[1] = (TO)hd[1];         d[2] = (TO)hd[3];
          d[3] = (TO)hd[1];         d[4] = (TO)(hd[2] + add); d[5] = (TO)hd[4];
          d[6] = (TO)hd[3];         d[7] = (TO)hd[4];         d[8] = (TO)(hd[5] + add);
        } else {
          d[0] = (TO)(hd[0] + add); d[1] = (TO)hd[1];
          d[2] = (TO)hd[1];         d[3] = (TO)(hd[2] + add);
        }
      } else {
        int t = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int j = 0; j <= i; j++) {
            const T v = hd[t++] + (i == j ? add : (T)0);
            if constexpr (LM) {   // a landmark's block is 3 x 3 row-major; its sums beyond are zero and go nowhere
              if (i < nd) {
                d[i * nd + j] = (TO)v;
                d[j * nd + i] = (TO)v;
              }
            } else {
            d[i * 6 + j] = (TO)v;
            d[j * 6 + i] = (TO)v;
            }
          }
      }
      TO *bo = a.b + a.node_offset[node];
#pragma unroll
      for (int t = 0; t < D; t++)
        if (t < nd) bo[t] = (TO)(-bv[t]);
      // rr_pgo_set_fixed: a fixed node's group has walked its incidences and priors as ever (the chi2 terms of its from-role
      // edges and of its priors count, it owns off-diagonal stores); what it just stored -- edge and prior terms, lambda, the
      // anchor term -- is overwritten with the identity block and b = 0
      if (fx_self) {
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
          for (int j = 0; j < D; j++)
            if (i < nd && j < nd) d[i * nd + j] = i == j ? (TO)1 : (TO)0;
#pragma unroll
        for (int t = 0; t < D; t++)
          if (t < nd) bo[t] = (TO)0;
      }
    }
  }
  double tot = block_sum<double, LIN_THREADS>(chi, red);
  if (threadIdx.x == 0) a.chi2_partial[blockIdx.x] = tot;
  opt_publish_chi2_in_last_block(a, lin_pre, red);
