// The RCCL communicator of a handle (metric reduction across ranks).  Included by muavta_kernels.hip.
extern "C" {

// ---- RCCL, loaded on first use --------------------------------------------------------------------------------
namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string err;
};
Rccl* rccl() {
  static Rccl R;
  if (R.lib || !R.err.empty()) return &R;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names) if ((R.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;   // a copy already in the process (PyTorch's)
  if (!R.lib) for (const char* n : names) if ((R.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
  if (!R.lib) { R.err = std::string("librccl not found: ") + dlerror(); return &R; }
  *(void**)&R.GetUniqueId = dlsym(R.lib, "ncclGetUniqueId");
  *(void**)&R.CommInitRank = dlsym(R.lib, "ncclCommInitRank");
  *(void**)&R.CommDestroy = dlsym(R.lib, "ncclCommDestroy");
  *(void**)&R.AllReduce = dlsym(R.lib, "ncclAllReduce");
  *(void**)&R.AllGather = dlsym(R.lib, "ncclAllGather");
  *(void**)&R.GetErrorString = dlsym(R.lib, "ncclGetErrorString");
  if (!R.GetUniqueId || !R.CommInitRank || !R.CommDestroy || !R.AllReduce || !R.AllGather || !R.GetErrorString) { R.err = "librccl lacks an expected symbol"; R.lib = nullptr; }
  return &R;
}
}  // namespace
#define NCCLCHK(env, expr)                                                                        \
  do {                                                                                            \
    ncclResult_t r_ = (expr);                                                                     \
    if (r_ != ncclSuccess) { (env)->err = std::string(#expr) + ": " + rccl()->GetErrorString(r_); return MUAVTA_E_HIP; } \
  } while (0)

int muavta_comm_uid(uint8_t* uid) {
  if (!uid) return MUAVTA_E_ARG;
  Rccl* R = rccl();
  if (!R->lib) { g_create_error = R->err; return MUAVTA_E_NO_DEVICE; }
  static_assert(sizeof(ncclUniqueId) == MUAVTA_COMM_UID_BYTES, "RCCL unique id size");
  ncclUniqueId id;
  ncclResult_t r = R->GetUniqueId(&id);
  if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + R->GetErrorString(r); return MUAVTA_E_HIP; }
  memcpy(uid, &id, sizeof(id));
  return MUAVTA_OK;
}
int muavta_comm_init(MuavtaEnv* e, int32_t rank, int32_t n_ranks, const uint8_t* uid) {
  if (!e || !uid || n_ranks < 1 || rank < 0 || rank >= n_ranks) { if (e) e->err = "muavta_comm_init: bad arguments"; return MUAVTA_E_ARG; }
  if (e->comm) { e->err = "muavta_comm_init: this handle already has a communicator"; return MUAVTA_E_STATE; }
  Rccl* R = rccl();
  if (!R->lib) { e->err = R->err; return MUAVTA_E_NO_DEVICE; }
  DeviceScope scope_(e->device);
  ncclUniqueId id;
  memcpy(&id, uid, sizeof(id));
  // staging first: a failure below must not leave a communicator behind that has nowhere to stage (a retry would be refused
  // as "already has a communicator" and the next all-reduce would touch a null buffer)
  DevBuf<void> staging;
  HIPCHK(e, staging.alloc((size_t)(64 + 64 * n_ranks + 128) * 8));
  ncclComm_t comm = nullptr;
  const ncclResult_t r = R->CommInitRank(&comm, n_ranks, id, rank);
  if (r != ncclSuccess) {
    e->err = std::string("ncclCommInitRank: ") + R->GetErrorString(r);
    return MUAVTA_E_HIP;
  }
  e->comm = comm; e->d_comm = std::move(staging);
  e->comm_rank = rank; e->comm_ranks = n_ranks;
  return MUAVTA_OK;
}
int muavta_allreduce_metrics(MuavtaEnv* e, const double* f_partials, int32_t nf, const int64_t* counters, int32_t nc, double* f_total, int64_t* c_total) {
  if (!e || nf < 0 || nc < 0 || nf > 64 || nc > 64 || (nf && (!f_partials || !f_total)) || (nc && (!counters || !c_total))) { if (e) e->err = "muavta_allreduce_metrics: bad arguments"; return MUAVTA_E_ARG; }
  if (!e->comm) { e->err = "muavta_allreduce_metrics before muavta_comm_init"; return MUAVTA_E_STATE; }
  Rccl* R = rccl();
  DeviceScope scope_(e->device);
  const int n = e->comm_ranks;
  double* fs = (double*)e->d_comm.p; double* fr = fs + 64;
  int64_t* cs = (int64_t*)(fr + (size_t)64 * n); int64_t* cr = cs + 64;
  if (nf) {
    HIPCHK(e, hipMemcpyAsync(fs, f_partials, (size_t)nf * 8, hipMemcpyHostToDevice, e->stream));
    NCCLCHK(e, R->AllGather(fs, fr, (size_t)nf, ncclDouble, e->comm, e->stream));
  }
  if (nc) {
    HIPCHK(e, hipMemcpyAsync(cs, counters, (size_t)nc * 8, hipMemcpyHostToDevice, e->stream));
    NCCLCHK(e, R->AllReduce(cs, cr, (size_t)nc, ncclInt64, ncclSum, e->comm, e->stream));
  }
  std::vector<double> gathered((size_t)nf * n);
  if (nf) HIPCHK(e, hipMemcpyAsync(gathered.data(), fr, gathered.size() * 8, hipMemcpyDeviceToHost, e->stream));
  if (nc) HIPCHK(e, hipMemcpyAsync(c_total, cr, (size_t)nc * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (int k = 0; k < nf; k++) {  // rank order: the same bits on every rank, whatever the ring order
    double s = 0.0;
    for (int r = 0; r < n; r++) s += gathered[(size_t)r * nf + k];
    f_total[k] = s;
  }
  return MUAVTA_OK;
}
int muavta_comm_destroy(MuavtaEnv* e) {
  if (!e) return MUAVTA_E_ARG;
  if (e->comm) {
    DeviceScope scope_(e->device);
    hipStreamSynchronize(e->stream);
    rccl()->CommDestroy(e->comm);
    e->comm = nullptr;
    e->d_comm.reset();
  }
  return MUAVTA_OK;
}

}  // extern "C"
