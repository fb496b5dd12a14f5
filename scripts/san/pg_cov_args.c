/* Host-side sanitizer driver for the request validation of slam_pg_covariance /
 * slam_pg_gate (test infrastructure only), in the manner of abi_args.c.
 *
 * Linked against capi.hip and posegraph_se3.hip built with `hipcc -Xarch_host
 * -fsanitize=address,undefined` (scripts/san/build_pg_cov_asan.sh): the host
 * half -- the schedule check, the walk over the host copy of the request, the
 * column count and the workspace arithmetic -- runs under ASan/UBSan.  The
 * problem is a 12-pose chain whose host tables are real (built below as
 * slam355.posegraph.pg_schedule builds them) and sit in exact-size heap blocks,
 * so a read past a list's end is reported.  Every call must be refused before
 * anything is launched, or be a pure size query; the device pointers are host
 * scratch no kernel may ever see.  Refuses to run where a GPU is visible. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slam355.h"

static int fails = 0, checks = 0;
static unsigned char scratch[1 << 12];
#define P ((void*)scratch)
#define HUGE_WS (1ll << 40)

static void expect_rc(int rc, int want, const char* what) {
  ++checks;
  const char* e = slam_last_error();
  if (rc != want || !e || !*e) {
    fprintf(stderr, "FAIL %s: rc=%d err='%s'\n", what, rc, e ? e : "(null)");
    ++fails;
  }
}
static void expect(int ok, const char* what) {
  ++checks;
  if (!ok) {
    fprintf(stderr, "FAIL %s\n", what);
    ++fails;
  }
}

enum { N = 12, E = 11, T = 2 };

/* the schedule of the chain 0-1-...-11: two tile rows, three stored tiles */
static int32_t* chain_schedule(int* len) {
  const int total = 16 + T + (T + 1) + (N + 1) + 2 * E + (E + 1) + 2 * E + E + (T + 1) + (T + 1) + 1 + 2;
  int32_t* s = (int32_t*)malloc(sizeof(int32_t) * total);
  int o = 0;
  const int32_t hdr[16] = {0x50473031, N, E, T, E, 3, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0};
  memcpy(s, hdr, sizeof hdr);
  o = 16;
  s[o++] = 0, s[o++] = 0;                       /* first */
  s[o++] = 0, s[o++] = 1, s[o++] = 3;           /* rowoff */
  s[o++] = 0;                                   /* pose_ptr */
  for (int i = 0; i < N; ++i) s[o] = s[o - 1] + ((i == 0 || i == N - 1) ? 1 : 2), ++o;
  for (int i = 0; i < N; ++i) {                 /* pose_ent: 2 edge + side, edge order */
    if (i > 0) s[o++] = 2 * (i - 1) + 1;
    if (i < N - 1) s[o++] = 2 * i;
  }
  for (int q = 0; q <= E; ++q) s[o++] = q;      /* pair_ptr */
  for (int q = 0; q < E; ++q) s[o++] = q, s[o++] = q + 1;  /* pair_ij */
  for (int q = 0; q < E; ++q) s[o++] = 2 * q;   /* pair_ent */
  s[o++] = 0, s[o++] = 1, s[o++] = 1;           /* col_ptr */
  s[o++] = 0, s[o++] = 1, s[o++] = 1;           /* upd_ptr */
  s[o++] = 1;                                   /* panel rows of column 0 */
  s[o++] = 1, s[o++] = 1;                       /* its update pair */
  if (o != total) {
    fprintf(stderr, "pg_cov_args: schedule of %d ints, expected %d\n", o, total);
    exit(2);
  }
  *len = total;
  return s;
}

static int32_t* list_of(const int32_t* v, int n) { /* an exact-size heap copy */
  int32_t* p = (int32_t*)malloc(sizeof(int32_t) * 2 * (n > 0 ? n : 1));
  memcpy(p, v, sizeof(int32_t) * 2 * (n > 0 ? n : 0));
  return p;
}

static int cov(const slam_pg_problem* pr, const int32_t* host, int n, double tol, long long ws_len) {
  return slam_pg_covariance(pr, P, host, n, tol, P, P, ws_len, P, NULL);
}
static int gate(const slam_pg_problem* pr, const int32_t* host, int n, double tol, long long ws_len) {
  return slam_pg_gate(pr, P, host, P, NULL, n, tol, P, P, P, P, ws_len, P, NULL);
}

int main(void) {
  if (slam_device_count() != 0) {
    fprintf(stderr, "pg_cov_args: a GPU is visible; this driver runs on the CPU host only\n");
    _Exit(2);
  }
  int sched_len = 0;
  int32_t* sched = chain_schedule(&sched_len);
  int32_t* edges = (int32_t*)malloc(sizeof(int32_t) * 2 * E);
  for (int k = 0; k < E; ++k) edges[2 * k] = k, edges[2 * k + 1] = k + 1;
  slam_pg_problem pr;
  memset(&pr, 0, sizeof pr);
  pr.n_poses = N, pr.n_edges = E, pr.loss = 0, pr.sched_len = sched_len, pr.loss_scale = 1.0;
  pr.poses[0] = pr.poses[1] = P;
  pr.edge_ij = P, pr.meas = P, pr.sqrt_info = P, pr.sched = P, pr.ws = P, pr.state = P;
  pr.edge_ij_host = edges, pr.sched_host = sched;
  pr.ws_len = slam_pg_workspace_len(N, E, 3);
  expect(pr.ws_len > 0, "pg workspace len");

  const long long w1 = slam_pg_cov_workspace_len(N, 1), w2 = slam_pg_cov_workspace_len(N, 2);
  expect(w1 > 2 * 4096 && w2 - w1 == 2 * 4096, "cov workspace len");
  expect_rc((int)slam_pg_cov_workspace_len(N, 3), SLAM_ERR_ARG, "cov ws: n_cols > T");
  expect_rc((int)slam_pg_cov_workspace_len(N, 0), SLAM_ERR_ARG, "cov ws: n_cols 0");
  expect_rc((int)slam_pg_cov_workspace_len(0, 1), SLAM_ERR_ARG, "cov ws: n_poses 0");
  expect_rc((int)slam_pg_cov_workspace_len(-2147483647 - 1, 1), SLAM_ERR_ARG, "cov ws: INT_MIN poses");
  expect_rc((int)slam_pg_cov_workspace_len(2147483647, 1), SLAM_ERR_ARG, "cov ws: INT_MAX poses");

  /* a valid request passes every check up to the workspace: two columns need w2 */
  const int32_t two[] = {0, 0, 3, 11, 11, 3, 3, 11};
  int32_t* l4 = list_of(two, 4);
  expect_rc(cov(&pr, l4, 4, 1e-8, w2 - 1), SLAM_ERR_WORKSPACE, "cov: short workspace, 2 columns");
  expect_rc(cov(&pr, l4 + 2, 3, 1e-8, w1 - 1), SLAM_ERR_WORKSPACE, "cov: short workspace, 1 column");
  expect_rc(cov(&pr, l4, 4, 1e-8, 0), SLAM_ERR_WORKSPACE, "cov: workspace 0");
  expect_rc(cov(&pr, l4, 4, 1e-8, -5), SLAM_ERR_WORKSPACE, "cov: workspace < 0");
  expect_rc(gate(&pr, l4 + 2, 3, 1e-8, w2 - 1), SLAM_ERR_WORKSPACE, "gate: both poses' columns");
  expect_rc(gate(&pr, l4, 4, 1e-8, HUGE_WS), SLAM_ERR_ARG, "gate: i == j");
  /* counts, tolerances, null pointers */
  expect_rc(cov(&pr, l4, 0, 1e-8, HUGE_WS), SLAM_ERR_ARG, "cov: n 0");
  expect_rc(cov(&pr, l4, -4, 1e-8, HUGE_WS), SLAM_ERR_ARG, "cov: n < 0");
  expect_rc(gate(&pr, l4, -2147483647 - 1, 1e-8, HUGE_WS), SLAM_ERR_ARG, "gate: n INT_MIN");
  expect_rc(cov(&pr, l4, 4, 1.0, HUGE_WS), SLAM_ERR_ARG, "cov: rank_tol 1");
  expect_rc(cov(&pr, l4, 4, -1e-300, HUGE_WS), SLAM_ERR_ARG, "cov: rank_tol < 0");
  expect_rc(gate(&pr, l4 + 2, 3, __builtin_nan(""), HUGE_WS), SLAM_ERR_ARG, "gate: rank_tol NaN");
  expect_rc(cov(&pr, NULL, 4, 1e-8, HUGE_WS), SLAM_ERR_ARG, "cov: null host list");
  expect_rc(slam_pg_covariance(&pr, NULL, l4, 4, 1e-8, P, P, HUGE_WS, P, NULL), SLAM_ERR_ARG, "cov: null device list");
  expect_rc(slam_pg_covariance(&pr, P, l4, 4, 1e-8, NULL, P, HUGE_WS, P, NULL), SLAM_ERR_ARG, "cov: null output");
  expect_rc(slam_pg_covariance(&pr, P, l4, 4, 1e-8, P, NULL, HUGE_WS, P, NULL), SLAM_ERR_ARG, "cov: null workspace");
  expect_rc(slam_pg_covariance(&pr, P, l4, 4, 1e-8, P, P, HUGE_WS, NULL, NULL), SLAM_ERR_ARG, "cov: null status");
  expect_rc(slam_pg_gate(&pr, P, l4 + 2, NULL, NULL, 3, 1e-8, P, P, P, P, HUGE_WS, P, NULL), SLAM_ERR_ARG,
            "gate: null meas");
  expect_rc(slam_pg_gate(&pr, P, l4 + 2, P, NULL, 3, 1e-8, NULL, NULL, NULL, P, HUGE_WS, P, NULL), SLAM_ERR_ARG,
            "gate: null outputs");
  expect_rc(slam_pg_covariance(NULL, P, l4, 4, 1e-8, P, P, HUGE_WS, P, NULL), SLAM_ERR_ARG, "cov: null problem");
  /* indices: the last entry of an exact-size list is the bad one */
  const int32_t bads[][2] = {{0, 12}, {12, 0}, {-1, 3}, {3, -1}, {2147483647, 0}, {0, -2147483647 - 1}};
  for (unsigned b = 0; b < sizeof bads / sizeof bads[0]; ++b) {
    int32_t v[6] = {3, 11, 0, 0, bads[b][0], bads[b][1]};
    int32_t* l = list_of(v, 3);
    expect_rc(cov(&pr, l, 3, 1e-8, HUGE_WS), SLAM_ERR_ARG, "cov: index out of range");
    v[2] = 1;
    memcpy(l, v, sizeof v);
    expect_rc(gate(&pr, l, 3, 1e-8, HUGE_WS), SLAM_ERR_ARG, "gate: index out of range");
    free(l);
  }
  /* what pg_check refuses reaches these entry points too */
  pr.ws_len -= 1;
  expect_rc(cov(&pr, l4, 4, 1e-8, HUGE_WS), SLAM_ERR_WORKSPACE, "cov: the problem's own workspace short");
  pr.ws_len += 1;
  sched[5] += 1;
  expect_rc(gate(&pr, l4 + 2, 3, 1e-8, HUGE_WS), SLAM_ERR_ARG, "gate: wrong schedule");
  sched[5] -= 1;
  pr.sched_len -= 1;
  expect_rc(cov(&pr, l4, 4, 1e-8, HUGE_WS), SLAM_ERR_ARG, "cov: schedule length");
  pr.sched_len += 1;

  free(l4);
  free(edges);
  free(sched);
  printf("pg_cov_args: %d checks, %d failed\n", checks, fails);
  return fails ? 1 : 0;
}
