// Stand-alone device probes of the C ABI (no handle).  Included by muavta_kernels.hip.
// The probes have no handle: they report through the thread's create error, and their device temporaries go with their owners.
#define CK(expr) HIPCHK_G(expr, (void)0)
static int probe_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_error = std::string(who) + ": no HIP device"; return MUAVTA_E_NO_DEVICE; }
  return MUAVTA_OK;
}

// muavta_domain_*: upload the `in` arrays of n doubles, launch (the device arrays, inputs first), download the `out` arrays
template <int NI, int NO, class Launch>
static int domain_probe(const char* who, int device, const double* const (&in)[NI], double* const (&out)[NO], int n, Launch launch) {
  if (int rc = probe_device(who)) return rc;
  for (const double* q : in) if (!q) return MUAVTA_E_ARG;
  for (double* q : out) if (!q) return MUAVTA_E_ARG;
  if (n < 1) return MUAVTA_E_ARG;
  DeviceScope scope_(device);
  DevBuf<double> d[NI + NO];
  const size_t bytes = (size_t)n * sizeof(double);
  for (DevBuf<double>& q : d) CK(q.alloc(bytes));
  for (int i = 0; i < NI; i++) CK(hipMemcpy(d[i], in[i], bytes, hipMemcpyHostToDevice));
  launch(d);
  CK(hipGetLastError());
  for (int i = 0; i < NO; i++) CK(hipMemcpy(out[i], d[NI + i], bytes, hipMemcpyDeviceToHost));
  return MUAVTA_OK;
}

extern "C" {

int muavta_lsap(int32_t device, const double* cost, int32_t n, int32_t nr, int32_t nc, int64_t* row, int64_t* col) {
  return muavta_lsap_impl(device, cost, n, nr, nc, row, col, MUAVTA_LSAP_AUTO);
}
int muavta_lsap_impl(int32_t device, const double* cost, int32_t n, int32_t nr, int32_t nc, int64_t* row, int64_t* col, int32_t impl) {
  if (int rc = probe_device("muavta_lsap")) return rc;
  if (!cost || !row || !col || n < 1 || nr < 1 || nc < 1) { g_create_error = "muavta_lsap: bad arguments"; return MUAVTA_E_ARG; }
  int mn = nr < nc ? nr : nc, mx = nr < nc ? nc : nr;
  if (mn > Tile64::A || mx > Tile64::T) { g_create_error = "muavta_lsap: at most 64 x 128"; return MUAVTA_E_ARG; }
  // scipy.optimize.linear_sum_assignment raises ValueError("matrix contains invalid numeric entries") for NaN / -inf
  for (size_t i = 0, m = (size_t)n * nr * nc; i < m; i++)
    if (std::isnan(cost[i]) || cost[i] == -INFINITY) { g_create_error = "muavta_lsap: matrix contains invalid numeric entries (NaN or -inf)"; return MUAVTA_E_ARG; }
  const bool fits_reg = mn <= TileLsapReg::A && mx <= TileLsapReg::T;
  if (impl < MUAVTA_LSAP_AUTO || impl > MUAVTA_LSAP_TILE64 || (impl == MUAVTA_LSAP_REGISTERS && !fits_reg)) {
    g_create_error = "muavta_lsap_impl: unknown solver, or problem beyond 32 x 64 for the register solver"; return MUAVTA_E_ARG;
  }
  // the env tiles' own solvers: min(nr, nc) <= agents, max(nr, nc) <= task slots of the tile
  const int tile_a = impl == MUAVTA_LSAP_TILE16 ? Tile16::A : impl == MUAVTA_LSAP_TILE24 ? Tile24::A : Tile64::A;
  const int tile_t = impl == MUAVTA_LSAP_TILE16 ? Tile16::T : impl == MUAVTA_LSAP_TILE24 ? Tile24::T : Tile64::T;
  if (impl >= MUAVTA_LSAP_TILE16 && (mn > tile_a || mx > tile_t)) {
    g_create_error = "muavta_lsap_impl: problem beyond " + std::to_string(tile_a) + " x " + std::to_string(tile_t) + " for the " +
                     std::to_string(tile_a) + "-agent tile's solver";
    return MUAVTA_E_ARG;
  }
  const bool use_reg = impl == MUAVTA_LSAP_REGISTERS || (impl == MUAVTA_LSAP_AUTO && fits_reg);
  DeviceScope scope_(device);
  DevBuf<double> dc; DevBuf<int64_t> dr, dcl; DevBuf<int32_t> dst;
  size_t cb = (size_t)n * nr * nc * sizeof(double), rb = (size_t)n * mn * sizeof(int64_t);
  CK(dc.alloc(cb)); CK(dr.alloc(rb)); CK(dcl.alloc(rb)); CK(dst.alloc((size_t)n * sizeof(int32_t)));
  CK(hipMemcpy(dc, cost, cb, hipMemcpyHostToDevice));
  auto launch_tile = [&](auto tile) -> hipError_t {  // k_lsap_tile<TL> for the env tile type of `tile`
    typedef decltype(tile) TL;
    size_t lds = Lds<TL>::bytes();
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lsap_tile<TL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
    hipLaunchKernelGGL((k_lsap_tile<TL>), dim3(n), dim3(WG), lds, 0, dc.p, nr, nc, dr.p, dcl.p, dst.p);
    return hipSuccess;
  };
  if (impl == MUAVTA_LSAP_TILE16) { CK(launch_tile(Tile16())); }
  else if (impl == MUAVTA_LSAP_TILE24) { CK(launch_tile(Tile24())); }
  else if (impl == MUAVTA_LSAP_TILE64) { CK(launch_tile(Tile64())); }
  else if (use_reg) {
    size_t lds = Lds<TileLsapReg>::bytes();
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lsap<TileLsapReg, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_lsap<TileLsapReg, true>), dim3(n), dim3(WG), lds, 0, dc.p, nr, nc, dr.p, dcl.p, dst.p);
  } else {
    size_t lds = Lds<TileLsapLds>::bytes();
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lsap<TileLsapLds, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_lsap<TileLsapLds, false>), dim3(n), dim3(WG), lds, 0, dc.p, nr, nc, dr.p, dcl.p, dst.p);
  }
  CK(hipGetLastError());
  std::vector<int32_t> status((size_t)n);
  CK(hipMemcpy(status.data(), dst, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(row, dr, rb, hipMemcpyDeviceToHost));
  CK(hipMemcpy(col, dcl, rb, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++)
    if (status[(size_t)i]) {  // scipy: ValueError("cost matrix is infeasible")
      g_create_error = "muavta_lsap: cost matrix " + std::to_string(i) + " is infeasible";
      return MUAVTA_E_ARG;
    }
  return MUAVTA_OK;
}

int muavta_domain_math(int32_t device, const double* x, const double* y, int32_t n, double* out_sqrt, double* out_div, double* out_div_neg) {
  const double* in[2] = {x, y};
  double* out[3] = {out_sqrt, out_div, out_div_neg};
  return domain_probe("muavta_domain_math", device, in, out, n, [n](DevBuf<double>* d) {
    hipLaunchKernelGGL(k_domain_math, dim3((n + 255) / 256), dim3(256), 0, 0, d[0].p, d[1].p, n, d[2].p, d[3].p, d[4].p); });
}
int muavta_domain_log(int32_t device, const double* x, int32_t n, double* out) {
  const double* in[1] = {x};
  double* outs[1] = {out};
  return domain_probe("muavta_domain_log", device, in, outs, n, [n](DevBuf<double>* d) {
    hipLaunchKernelGGL(k_libm_log, dim3((n + 255) / 256), dim3(256), 0, 0, d[0].p, n, d[1].p); });
}
int muavta_domain_atan2(int32_t device, const double* y, const double* x, int32_t n, double* out) {
  const double* in[2] = {y, x};
  double* outs[1] = {out};
  return domain_probe("muavta_domain_atan2", device, in, outs, n, [n](DevBuf<double>* d) {
    hipLaunchKernelGGL(k_libm_atan2, dim3((n + 255) / 256), dim3(256), 0, 0, d[0].p, d[1].p, n, d[2].p); });
}

int muavta_avoid_obstacles(int32_t device, const double* agent_pos, const double* movement, int32_t n, const double* obstacles,
                           int32_t n_obstacles, double* out) {
  if (int rc = probe_device("muavta_avoid_obstacles")) return rc;
  if (!agent_pos || !movement || !out || n < 1 || n_obstacles < 0 || (n_obstacles > 0 && !obstacles)) return MUAVTA_E_ARG;
  DeviceScope scope_(device);
  DevBuf<double> dp, dm, dob, dout;
  CK(dp.alloc((size_t)n * 16)); CK(dm.alloc((size_t)n * 16)); CK(dout.alloc((size_t)n * 16));
  CK(dob.alloc((size_t)(n_obstacles > 0 ? n_obstacles : 1) * 24));
  CK(hipMemcpy(dp, agent_pos, (size_t)n * 16, hipMemcpyHostToDevice));
  CK(hipMemcpy(dm, movement, (size_t)n * 16, hipMemcpyHostToDevice));
  if (n_obstacles > 0) CK(hipMemcpy(dob, obstacles, (size_t)n_obstacles * 24, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_avoid, dim3((n + 255) / 256), dim3(256), 0, 0, dp.p, dm.p, n, dob.p, n_obstacles, dout.p);
  CK(hipGetLastError());
  CK(hipMemcpy(out, dout, (size_t)n * 16, hipMemcpyDeviceToHost));
  return MUAVTA_OK;
}
#undef CK

}  // extern "C"
