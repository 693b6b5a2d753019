// The transport's interface (qg_comm.hip): the y-slab ring of one rank per GPU, over RCCL or the
// caller's host callbacks.  Declared once, here; qg_comm.hip includes it, so the compiler holds
// every definition to its declaration.  `comm` / `user` is the handle comm_init* made.
#pragma once

#include "qg_common.hpp"

namespace qg {

int comm_unique_id(char out[128]);
int comm_init(void **comm, int nranks, int rank, const char id[128]);
int comm_init_host(void **comm, int nranks, int rank, qg_allgather_fn ag, qg_sendrecv_fn sr, void *user);
int comm_destroy(void *comm);
// Bounded host wait on a stream (ev == nullptr) or an event, for a context with a transport
// attached (comm != nullptr): fails with QG_ERR_RCCL on an RCCL async error or when no halo
// exchange completes within the transport's timeout.  comm == nullptr: a plain
// hipStreamSynchronize / hipEventSynchronize.
int comm_wait(void *comm, hipStream_t s, hipEvent_t ev, const char *what);
int comm_set_timeout(void *comm, double seconds);
int comm_allgather(void *user, const double *send, double *recv, int64_t count, hipStream_t s);
int comm_gather_records(void *user, const double *send, double *recv, int64_t count, hipStream_t s);
int comm_halo(void *comm, double *const *fields, int nfields, int64_t M, int64_t P, int depth, double *halo_buf,
              hipStream_t s);
int comm_halo_rows(void *comm, double *const *f2, int n2, int64_t ld, int64_t P, hipStream_t s,
                   const double **rows_out);
int comm_exchange(void *comm, double *const *f2, int n2, double *halo_buf, double *const *f1, int n1, int64_t ld,
                  int64_t P, hipStream_t s, bool ghost_f2);
int comm_set_peer(void *comm, int on, int64_t ld);
int comm_set_peer_gather(void *comm, int on, int64_t count);

}  // namespace qg
