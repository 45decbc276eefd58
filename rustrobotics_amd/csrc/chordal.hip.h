// chordal.hip.h -- rr_pgo_initialize: the chordal relaxation (Carlone, Tron, Daniilidis, Dellaert, ICRA 2015).
// Three kernels; the factorisation and the back substitution between them are the handle's own (pgo_api.hip, Engine::initialize).
//
//   k_chordal_lin      H and b of one relaxed LINEAR problem, in the block layout of k_linearize (same pattern, same slots):
//                        STAGE 0   2-D: u = (cos, sin) of every pose, block (c, s, .)
//                                  3-D: rows 1 and 2 of every pose's relaxed rotation M, block (rho1, rho2)
//                        STAGE 1   3-D: row 3, block (rho3, . . .)
//                        STAGE 2   positions, block (t, .) of a pose, l of a landmark
//                      "." is a dummy scalar: diagonal 1, right-hand side 0, every off-diagonal entry 0.  A landmark's block in
//                      a rotation stage and the block of a HELD node (fixed, or the kept anchor) in every stage is the identity
//                      with b = 0 and zero off-diagonal blocks, the layout of rr_pgo_set_fixed; a held node's value moves into
//                      its free neighbours' right-hand sides.
//   k_chordal_project  M_i -> the nearest rotation (3-D: R = U diag(1, 1, det(U V^T)) V^T; 2-D: u / |u|), per pose, into a
//                      scratch buffer; a held pose's rotation is copied from the state
//   k_chordal_place    the state of every free node from the position solve and the projected rotations
//
// With rho^k the k-th row of M as a column, an SE3 edge (i, j) with measured rotation R_ij says rho_j = R_ij^T rho_i; in 2-D
// u_j = Rot(theta_ij) u_i.  Both are rho_j = A rho_i with an orthogonal A, so the normal equations of
// kappa |A rho_i - rho_j|^2 are  H_ii += kappa I,  H_jj += kappa I,  H_ij = -kappa A^T.
// A position term |R_i^T (t_j - t_i) - z|^2_Omega is (t_j - t_i - d)^T W (t_j - t_i - d) with W = R_i Omega R_i^T, d = R_i z:
// H_ii += W, H_jj += W, H_ij = -W, b_i -= W d, b_j += W d.
#pragma once

namespace rrpgo {

template <typename T, typename TC = T> struct ChordalArgs {
  int n_nodes;
  const typename VecT<TC>::V4 *pose;     // the state (read only: held values)
  const EdgeRec<TC> *e_rec;              // SE(2)
  const typename VecT<TC>::V4 *e_meas;   // SE(3)
  const TC *e_info;
  const int64_t *e_slot;
  const int32_t *inc_ptr;
  const int2 *inc_list;
  const uint8_t *node_dim;
  const int32_t *node_offset;
  const int64_t *diag_off;
  T *hvals;
  T *b;
  unsigned *zero_words;                  // as LinArgs: flags and tickets of the dataflow launches that follow
  int n_zero_words;
  unsigned *fill_words;                  // as LinArgs: the solution vector of k_solve_flow
  int n_fill_words;
  const int32_t *prior_ptr;              // null: no priors
  const EdgeRec<TC> *prior_rec;
  const typename VecT<TC>::V4 *prior_meas;
  const TC *prior_info;
  const uint8_t *fixed;                  // null: none
  int anchor;                            // the held anchor, -1: not held
  const TC *rot;                         // STAGE 2: k_chordal_project's result, 2 (2-D) or 9 (3-D, row-major) scalars per node
};

template <typename A> __device__ __forceinline__ bool chordal_held(const A &a, int node) {
  return node == a.anchor || (a.fixed && a.fixed[node]);
}

// the SD x SD orthogonal matrix of a packed pose or measurement: Rot(theta) from (cos, sin), R(q)
template <typename T> __device__ __forceinline__ void chordal_rot2(T c, T s, T (&R)[2][2]) {
  R[0][0] = c; R[0][1] = -s;
  R[1][0] = s; R[1][1] = c;
}

template <typename TO, typename T, int D, int STAGE>
__global__ void __launch_bounds__(LIN_THREADS) k_chordal_lin(ChordalArgs<TO, T> a) {
  using V4 = typename VecT<T>::V4;
  constexpr int SD = D == 3 ? 2 : 3;                           // space dimension: a landmark's block, a position
  constexpr bool ROT = STAGE < 2;
  constexpr int NRHO = (D == 6 && STAGE == 0) ? 2 : 1;         // rows of M this rotation stage solves for
  constexpr int ROW0 = (D == 6 && STAGE == 1) ? 2 : 0;         // ... the first of them
  constexpr int NL = ROT ? NRHO * SD : SD;                     // live scalars of a pose's block; the rest are dummies
  constexpr int NV = D / 3;
  const int gid = blockIdx.x * LIN_THREADS + threadIdx.x;
  for (int i = gid; i < a.n_zero_words; i += gridDim.x * LIN_THREADS) a.zero_words[i] = 0u;
  for (int i = gid; i < a.n_fill_words; i += gridDim.x * LIN_THREADS) a.fill_words[i] = X_PENDING_WORD;
  const int slot = gid / LIN_GROUP, sub = gid % LIN_GROUP;
  const int node = slot < a.n_nodes ? slot : -1;
  T kap = 0;           // rotation stages: the diagonal is kap I
  T hd[SD][SD];        // position stage: the diagonal block (full, symmetric)
  T bv[NL];
#pragma unroll
  for (int i = 0; i < SD; i++)
#pragma unroll
    for (int j = 0; j < SD; j++) hd[i][j] = 0;
#pragma unroll
  for (int t = 0; t < NL; t++) bv[t] = 0;
  int nd = D;
  bool held = false;
  if (node >= 0) {
    nd = a.node_dim[node];
    held = chordal_held(a, node);
    const int q1 = a.inc_ptr[node + 1];
    for (int q = a.inc_ptr[node] + sub; q < q1; q += LIN_GROUP) {
      const int2 inc = a.inc_list[q];
      const int ent = inc.x, k = ent >> 4, role = ent & 1;
      const bool lm_edge = (ent >> 1) & 1;
      const bool other_held = chordal_held(a, inc.y);
      // ---- per dimension: the operands
      V4 mz[NV], po[NV];
      T om[SD][SD];    // position stage: Omega_tt (a landmark edge: Omega)
      T kq = 0;        // rotation stages: kappa
      int64_t so;
      bool skip = false;   // the edge takes no part in this stage: its off-diagonal block is still zeroed
      if constexpr (D == 3) {
        const EdgeRec<T> rec = a.e_rec[k];
        mz[0] = rec.meas;
        so = rec.slot;
        po[0] = a.pose[inc.y];
        om[0][0] = rec.info_a.x; om[0][1] = rec.info_a.y;
        om[1][0] = rec.info_a.y; om[1][1] = rec.info_a.w;
        kq = rec.info_b.y;
        if (lm_edge && rec.meas.w != (T)0) skip = true;   // bearing-only / range-only: one scalar places nothing
      } else {
        mz[0] = a.e_meas[2 * k]; mz[1] = a.e_meas[2 * k + 1];
        so = a.e_slot[k];
        po[0] = a.pose[2 * inc.y]; po[1] = a.pose[2 * inc.y + 1];
        const T *w = a.e_info + (int64_t)k * 21;
        om[0][0] = w[0]; om[0][1] = w[1]; om[0][2] = w[2];
        om[1][0] = w[1]; om[1][1] = w[6]; om[1][2] = w[7];
        om[2][0] = w[2]; om[2][1] = w[7]; om[2][2] = w[11];
        kq = (w[15] + w[18] + w[20]) / (T)3;
      }
      if (ROT && lm_edge) skip = true;
      T off[SD][SD];   // the live SD x SD sub-block of H[from rows, to cols] (rotation stages: the same for every row of M)
#pragma unroll
      for (int i = 0; i < SD; i++)
#pragma unroll
        for (int j = 0; j < SD; j++) off[i][j] = 0;
      if (!skip) {
        if constexpr (ROT) {
          // rho_to = A rho_from
          T Am[SD][SD];
          if constexpr (D == 3) {
            chordal_rot2<T>(mz[0].z, mz[0].w, Am);
          } else {
            const T qz[4] = {mz[1].x, mz[1].y, mz[1].z, mz[1].w};
            T Rz[3][3];
            q_to_rot(qz, Rz);
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
              for (int j = 0; j < 3; j++) Am[i][j] = Rz[j][i];
          }
          kap += kq;
#pragma unroll
          for (int i = 0; i < SD; i++)
#pragma unroll
            for (int j = 0; j < SD; j++) off[i][j] = -kq * Am[j][i];
          if (other_held) {
            // the held neighbour's rows of R, as columns
            T Ro[SD][SD];
            if constexpr (D == 3) {
              Ro[0][0] = po[0].z; Ro[0][1] = po[0].w; Ro[1][0] = 0; Ro[1][1] = 0;   // (row 0 alone is read)
            } else {
              const T qo[4] = {po[1].x, po[1].y, po[1].z, po[1].w};
              q_to_rot(qo, Ro);
            }
#pragma unroll
            for (int r = 0; r < NRHO; r++)
#pragma unroll
              for (int i = 0; i < SD; i++) {
                T s = 0;
#pragma unroll
                for (int j = 0; j < SD; j++) s += (role ? Am[i][j] : Am[j][i]) * Ro[ROW0 + r][j];
                bv[r * SD + i] += kq * s;
              }
          }
        } else {
          // W = R_from Omega R_from^T, d = R_from z
          const int from = role ? inc.y : node;
          T Rf[SD][SD];
#pragma unroll
          for (int i = 0; i < SD; i++)
#pragma unroll
            for (int j = 0; j < SD; j++) Rf[i][j] = 0;
          if constexpr (D == 3) {
            chordal_rot2<T>(a.rot[2 * from], a.rot[2 * from + 1], Rf);
          } else {
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
              for (int j = 0; j < 3; j++) Rf[i][j] = a.rot[9 * (int64_t)from + 3 * i + j];
          }
          T RO[SD][SD], W[SD][SD];
#pragma unroll
          for (int i = 0; i < SD; i++)
#pragma unroll
            for (int j = 0; j < SD; j++) {
              T s = 0;
#pragma unroll
              for (int r = 0; r < SD; r++) s += Rf[i][r] * om[r][j];
              RO[i][j] = s;
            }
#pragma unroll
          for (int i = 0; i < SD; i++)
#pragma unroll
            for (int j = 0; j < SD; j++) {
              T s = 0;
#pragma unroll
              for (int r = 0; r < SD; r++) s += RO[i][r] * Rf[j][r];
              W[i][j] = s;
            }
          // what this node's equation has on its right: -+ d, and the held neighbour's position
          T zt[SD], rhs[SD];
          zt[0] = mz[0].x; zt[1] = mz[0].y;
          if constexpr (SD == 3) zt[2] = mz[0].z;
          T to[SD];
          to[0] = po[0].x; to[1] = po[0].y;
          if constexpr (SD == 3) to[2] = po[0].z;
#pragma unroll
          for (int i = 0; i < SD; i++) {
            T s = 0;
#pragma unroll
            for (int r = 0; r < SD; r++) s += Rf[i][r] * zt[r];
            rhs[i] = (role ? s : -s) + (other_held ? to[i] : (T)0);
          }
#pragma unroll
          for (int i = 0; i < SD; i++) {
            T s = 0;
#pragma unroll
            for (int j = 0; j < SD; j++) {
              s += W[i][j] * rhs[j];
              hd[i][j] += W[i][j];
              off[i][j] = -W[i][j];
            }
            bv[i] += s;
          }
        }
      }
      if (role == 0 && (ent & 8)) {
        // H[from rows, to cols]: D x D, or D x SD into a landmark; the live sub-blocks, zeros around them, zeros everywhere
        // when an endpoint is held
        TO *dst = a.hvals + (so >> 1);
        const bool tr = so & 1;
        const int d2 = lm_edge ? SD : D;
        const bool zero = held | other_held;
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
          for (int j = 0; j < D; j++) {
            if (j >= d2) continue;
            T v = 0;
            if constexpr (ROT) {
              if (i / SD == j / SD && i < NL) v = off[i % SD][j % SD];
            } else {
              if (i < SD && j < SD) v = off[i][j];
            }
            dst[tr ? j * D + i : i * d2 + j] = zero ? (TO)0 : (TO)v;
          }
      }
    }
    if (a.prior_ptr) {
      const int p1 = a.prior_ptr[node + 1];
      for (int p = a.prior_ptr[node] + sub; p < p1; p += LIN_GROUP) {
        V4 mz[NV];
        T om[SD][SD];
        T kq = 0;
        if constexpr (D == 3) {
          const EdgeRec<T> rec = a.prior_rec[p];
          mz[0] = rec.meas;
          om[0][0] = rec.info_a.x; om[0][1] = rec.info_a.y;
          om[1][0] = rec.info_a.y; om[1][1] = rec.info_a.w;
          kq = rec.info_b.y;
        } else {
          mz[0] = a.prior_meas[2 * p]; mz[1] = a.prior_meas[2 * p + 1];
          const T *w = a.prior_info + (int64_t)p * 21;
          om[0][0] = w[0]; om[0][1] = w[1]; om[0][2] = w[2];
          om[1][0] = w[1]; om[1][1] = w[6]; om[1][2] = w[7];
          om[2][0] = w[2]; om[2][1] = w[7]; om[2][2] = w[11];
          kq = (w[15] + w[18] + w[20]) / (T)3;
        }
        const bool on_pose = nd == D;
        // the measured rotation (a landmark's prior: the identity)
        T Rz[SD][SD];
#pragma unroll
        for (int i = 0; i < SD; i++)
#pragma unroll
          for (int j = 0; j < SD; j++) Rz[i][j] = i == j ? (T)1 : (T)0;
        if (on_pose) {
          if constexpr (D == 3) {
            chordal_rot2<T>(mz[0].z, mz[0].w, Rz);
          } else {
            const T qz[4] = {mz[1].x, mz[1].y, mz[1].z, mz[1].w};
            q_to_rot(qz, Rz);
          }
        }
        if constexpr (ROT) {
          if (on_pose) {
            kap += kq;
            if constexpr (D == 3) {
              bv[0] += kq * mz[0].z;
              bv[1] += kq * mz[0].w;
            } else {
#pragma unroll
              for (int r = 0; r < NRHO; r++)
#pragma unroll
                for (int i = 0; i < SD; i++) bv[r * SD + i] += kq * Rz[ROW0 + r][i];
            }
          }
        } else {
          T RO[SD][SD], W[SD][SD], zt[SD];
          zt[0] = mz[0].x; zt[1] = mz[0].y;
          if constexpr (SD == 3) zt[2] = mz[0].z;
#pragma unroll
          for (int i = 0; i < SD; i++)
#pragma unroll
            for (int j = 0; j < SD; j++) {
              T s = 0;
#pragma unroll
              for (int r = 0; r < SD; r++) s += Rz[i][r] * om[r][j];
              RO[i][j] = s;
            }
#pragma unroll
          for (int i = 0; i < SD; i++)
#pragma unroll
            for (int j = 0; j < SD; j++) {
              T s = 0;
#pragma unroll
              for (int r = 0; r < SD; r++) s += RO[i][r] * Rz[j][r];
              W[i][j] = s;
            }
#pragma unroll
          for (int i = 0; i < SD; i++) {
            T s = 0;
#pragma unroll
            for (int j = 0; j < SD; j++) {
              s += W[i][j] * zt[j];
              hd[i][j] += W[i][j];
            }
            bv[i] += s;
          }
        }
      }
    }
  }
  if constexpr (ROT) kap = group_sum8(kap);
  else {
#pragma unroll
    for (int i = 0; i < SD; i++)
#pragma unroll
      for (int j = 0; j < SD; j++) hd[i][j] = group_sum8(hd[i][j]);
  }
#pragma unroll
  for (int t = 0; t < NL; t++) bv[t] = group_sum8(bv[t]);
  if (node >= 0 && sub == 0) {
    // a held node, and a landmark in a rotation stage: the identity and b = 0
    const bool ident = held || (ROT && nd != D);
    TO *d = a.hvals + a.diag_off[node];
    TO *bo = a.b + a.node_offset[node];
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
      for (int j = 0; j < D; j++) {
        if (i >= nd || j >= nd) continue;
        T v = i == j ? (T)1 : (T)0;
        if (!ident) {
          if constexpr (ROT) {
            if (i == j && i < NL) v = kap;
          } else {
            // (symmetrised: the two triangles of R Omega R^T differ in their last bits)
            if (i < SD && j < SD) v = i <= j ? hd[i][j] : hd[j][i];
          }
        }
        d[i * nd + j] = (TO)v;
      }
#pragma unroll
    for (int t = 0; t < D; t++) {
      if (t >= nd) continue;
      T v = 0;
      if (!ident && t < NL) v = bv[t < NL ? t : 0];
      bo[t] = (TO)v;
    }
  }
}

// ---- the projection

// one Jacobi rotation of the symmetric 3 x 3 matrix A in the (P, Q) plane, accumulated into V (A = V diag V^T at the end);
// every index is a template argument: the arrays stay in registers
template <int P, int Q, typename T> __device__ __forceinline__ void chordal_jacobi(T (&A)[3][3], T (&V)[3][3]) {
  constexpr int R = 3 - P - Q;
  const T apq = A[P][Q];
  if (apq == (T)0) return;
  const T theta = (A[Q][Q] - A[P][P]) / ((T)2 * apq);
  const T t = (theta >= (T)0 ? (T)1 : (T)-1) / (fabs(theta) + sqrt(theta * theta + (T)1));
  const T c = (T)1 / sqrt(t * t + (T)1), s = t * c;
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = 0; A[Q][P] = 0;
  const T arp = A[R][P], arq = A[R][Q];
  A[R][P] = c * arp - s * arq; A[P][R] = A[R][P];
  A[R][Q] = s * arp + c * arq; A[Q][R] = A[R][Q];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const T vip = V[i][P], viq = V[i][Q];
    V[i][P] = c * vip - s * viq;
    V[i][Q] = s * vip + c * viq;
  }
}
// order eigenpairs P and Q by descending eigenvalue
template <int P, int Q, typename T> __device__ __forceinline__ void chordal_order(T (&lam)[3], T (&V)[3][3]) {
  if (lam[P] >= lam[Q]) return;
  const T l = lam[P]; lam[P] = lam[Q]; lam[Q] = l;
#pragma unroll
  for (int i = 0; i < 3; i++) { const T v = V[i][P]; V[i][P] = V[i][Q]; V[i][Q] = v; }
}

constexpr int CHORDAL_SWEEPS = 8;   // cyclic Jacobi converges quadratically: a 3 x 3 is at rounding level after 4 or 5 sweeps

// R = U diag(1, 1, det(U V^T)) V^T of M = U Sigma V^T, from the eigenvectors v1, v2 of M^T M of the two LARGEST eigenvalues:
// u1 = M v1 / |.|, u2 = M v2 orthonormalised against u1, and R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T -- the third pair comes
// from cross products, so the smallest singular value is never divided by and the determinant is +1 by construction.
template <typename T> __device__ __forceinline__ void chordal_project3(const T (&M)[3][3], T (&R)[3][3]) {
  T A[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      A[i][j] = M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j];
      V[i][j] = i == j ? (T)1 : (T)0;
    }
#pragma unroll 1
  for (int sweep = 0; sweep < CHORDAL_SWEEPS; sweep++) {
    chordal_jacobi<0, 1>(A, V);
    chordal_jacobi<0, 2>(A, V);
    chordal_jacobi<1, 2>(A, V);
  }
  T lam[3] = {A[0][0], A[1][1], A[2][2]};
  chordal_order<0, 1>(lam, V);
  chordal_order<1, 2>(lam, V);
  chordal_order<0, 1>(lam, V);
  T v1[3] = {V[0][0], V[1][0], V[2][0]}, v2[3] = {V[0][1], V[1][1], V[2][1]};
  T u1[3], u2[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    u1[i] = M[i][0] * v1[0] + M[i][1] * v1[1] + M[i][2] * v1[2];
    u2[i] = M[i][0] * v2[0] + M[i][1] * v2[1] + M[i][2] * v2[2];
  }
  const T n1 = (T)1 / sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  u1[0] *= n1; u1[1] *= n1; u1[2] *= n1;
  const T dp = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
  u2[0] -= dp * u1[0]; u2[1] -= dp * u1[1]; u2[2] -= dp * u1[2];
  const T n2 = (T)1 / sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  u2[0] *= n2; u2[1] *= n2; u2[2] *= n2;
  const T u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  const T v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R[i][j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
}

template <typename T, typename TC> struct ChordalNodeArgs {
  int n_nodes, is3d;
  typename VecT<TC>::V4 *pose;           // k_chordal_project reads it (held poses); k_chordal_place writes the free nodes
  const uint8_t *node_dim;
  const int32_t *node_offset;
  const uint8_t *fixed;
  int anchor;
  const T *sol_a;                        // exported solutions, reference order: project: stage 0; place: the position stage
  const T *sol_b;                        // project, 3-D: stage 1
  TC *rot;                               // 2 (2-D) or 9 (3-D, row-major) scalars per node; landmarks' entries are not touched
};

// one thread per pose
template <typename T, typename TC>
__global__ void __launch_bounds__(256) k_chordal_project(ChordalNodeArgs<T, TC> a) {
  const int node = blockIdx.x * 256 + threadIdx.x;
  if (node >= a.n_nodes) return;
  const bool held = chordal_held(a, node);
  if (!a.is3d) {
    if (a.node_dim[node] != 3) return;
    TC c, s;
    if (held) {
      const auto p = a.pose[node];
      c = p.z; s = p.w;
    } else {
      const T *x = a.sol_a + a.node_offset[node];
      c = (TC)x[0]; s = (TC)x[1];
      const TC inv = (TC)1 / sqrt(c * c + s * s);
      c *= inv; s *= inv;
    }
    a.rot[2 * node] = c;
    a.rot[2 * node + 1] = s;
    return;
  }
  if (a.node_dim[node] != 6) return;
  TC R[3][3];
  if (held) {
    const auto pq = a.pose[2 * node + 1];
    const TC q[4] = {pq.x, pq.y, pq.z, pq.w};
    q_to_rot(q, R);
  } else {
    const T *xa = a.sol_a + a.node_offset[node], *xb = a.sol_b + a.node_offset[node];
    const TC M[3][3] = {{(TC)xa[0], (TC)xa[1], (TC)xa[2]}, {(TC)xa[3], (TC)xa[4], (TC)xa[5]}, {(TC)xb[0], (TC)xb[1], (TC)xb[2]}};
    chordal_project3<TC>(M, R);
  }
  TC *dst = a.rot + 9 * (int64_t)node;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) dst[3 * i + j] = R[i][j];
}

// a rotation matrix as a unit quaternion with w >= 0 (the branch with the largest divisor)
template <typename T> __device__ __forceinline__ void chordal_rot_to_q(const T *R, T (&q)[4]) {
  const T r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
  const T tr = r00 + r11 + r22;
  T x, y, z, w;
  if (tr > (T)0) {
    const T s = (T)2 * sqrt(tr + (T)1);
    w = (T)0.25 * s; x = (r21 - r12) / s; y = (r02 - r20) / s; z = (r10 - r01) / s;
  } else if (r00 > r11 && r00 > r22) {
    const T s = (T)2 * sqrt((T)1 + r00 - r11 - r22);
    w = (r21 - r12) / s; x = (T)0.25 * s; y = (r01 + r10) / s; z = (r02 + r20) / s;
  } else if (r11 > r22) {
    const T s = (T)2 * sqrt((T)1 + r11 - r00 - r22);
    w = (r02 - r20) / s; x = (r01 + r10) / s; y = (T)0.25 * s; z = (r12 + r21) / s;
  } else {
    const T s = (T)2 * sqrt((T)1 + r22 - r00 - r11);
    w = (r10 - r01) / s; x = (r02 + r20) / s; y = (r12 + r21) / s; z = (T)0.25 * s;
  }
  const T inv = (w < (T)0 ? (T)-1 : (T)1) / sqrt(x * x + y * y + z * z + w * w);
  q[0] = x * inv; q[1] = y * inv; q[2] = z * inv; q[3] = w * inv;
}

// one thread per node; the only launch of rr_pgo_initialize that writes the state.  Held nodes are left alone.
template <typename T, typename TC>
__global__ void __launch_bounds__(256) k_chordal_place(ChordalNodeArgs<T, TC> a) {
  const int node = blockIdx.x * 256 + threadIdx.x;
  if (node >= a.n_nodes) return;
  if (chordal_held(a, node)) return;
  const T *x = a.sol_a + a.node_offset[node];
  const int nd = a.node_dim[node];
  if (!a.is3d) {
    auto p = a.pose[node];
    p.x = (TC)x[0]; p.y = (TC)x[1];
    if (nd == 3) { p.z = a.rot[2 * node]; p.w = a.rot[2 * node + 1]; }
    a.pose[node] = p;
    return;
  }
  auto pt = a.pose[2 * node];
  pt.x = (TC)x[0]; pt.y = (TC)x[1]; pt.z = (TC)x[2];
  a.pose[2 * node] = pt;
  if (nd == 6) {
    TC q[4];
    chordal_rot_to_q<TC>(a.rot + 9 * (int64_t)node, q);
    auto pq = a.pose[2 * node + 1];
    pq.x = q[0]; pq.y = q[1]; pq.z = q[2]; pq.w = q[3];
    a.pose[2 * node + 1] = pq;
  }
}

}  // namespace rrpgo
