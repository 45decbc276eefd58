// update_frame.inc -- the body of k_update and of k_update_lm (kernels.hip.h includes it inside each of the two kernels, behind
// `constexpr bool LM`; TO, T, D and the argument `a` are the kernel's).
  __shared__ double red[UPD_THREADS / 64];
  const int node = listed_node(a, blockIdx.x * UPD_THREADS + threadIdx.x);
  double nrm = 0.0;
  // rr_pgo_optimize: enqueued behind the iteration that met the stop rule (:298-300) -- the state, the partials, the slot
  // counter and the ring stay as that iteration left them
  if (opt_stopped(a.err)) return;
  if (a.gate && *a.gate == 0) return;
  const FinPre fin_pre = finalize_preload<UPD_THREADS>(a.fin);   // requested ahead of the node work
  const bool failed = a.err && a.err[0] != 0;   // a failed factorisation: the state stays
  if (node >= 0 && !failed) {
    if (a.fixed && a.fixed[node]) {
      // a fixed node is skipped, not updated with zero (SE(3) renormalises the quaternion): its state bits stay, it adds
      // nothing to |dx|^2 and the exported step is 0
      if (a.dx_ref_out) {
        int nd = D;
        if constexpr (D == 3 || LM) nd = a.node_dim[node];
        TO *dst = a.dx_ref_out + a.node_offset[node];
        for (int t = 0; t < nd; t++) dst[t] = (TO)0;
      }
    } else if constexpr (D == 3) nrm = update_node(a, node);
    else if constexpr (LM) nrm = a.node_dim[node] == 3 ? update_node_xyz(a, node) : update_node_se3(a, node);
    else nrm = update_node_se3(a, node);
  }
  if (a.export_only) return;
  double tot = block_sum<double, UPD_THREADS>(nrm, red);
  if (threadIdx.x == 0) a.norm_partial[blockIdx.x] = tot;
  if (a.fin.enabled) finalize_in_last_block<UPD_THREADS>(a.fin, fin_pre, a.norm_partial, (int)gridDim.x, red);
