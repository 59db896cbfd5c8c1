/* The library's environment switches: every read of an X265AMD_* variable in csrc/ and host/ goes through the functions below, and the list here is the only list.
 * (Host C++ only, nothing from HIP: host/xa_fiber.cpp includes it too.)  Where a switch is read -- once per process into a static, or at every call -- is the reader's
 * choice and written there; the ones marked "per call" are switched by tests inside one process.
 *
 * Diagnostics: they print, dump or verify, and decide nothing about the stream.
 *   X265AMD_TIMING          present        per-picture, per-row and per-stage wall times, the chains', searches-ahead's and scheduler's counters on stderr   DESIGN 5
 *   X265AMD_HOSTPROF        present | wall the XA_HOSTPROF scopes' totals at exit (wall: on the wall clock, parked time included)                            DESIGN 4.14
 *   X265AMD_QUEUE_PROF      present        the job server's per-command statistics and stage clocks                                                          DESIGN 4.29
 *   X265AMD_QUEUE_LOG       poc,row        the command / wait timeline of that CTU row's queue (dbg/qlog_report.py)                                          DESIGN 4.6
 *   X265AMD_QUEUE_TRACE     present | 2    names every queue command and waits for it (2: more of each)                                                      DESIGN 4.6
 *   X265AMD_QUEUE_DEBUG     bits           handed to every command (XaCmd::reserved); 2: what each wavefront was about to touch, dumped on SIGABRT            DESIGN 4.6
 *   X265AMD_CTU_LOG         present | pN   one line per CTU of the last three rows (pN: of every row of picture N) with its waits by class (dbg/ctu_grid.py) DESIGN 4.21
 *   X265AMD_CHAIN_LOG       x,y            the results of the intra chains of the 16x16 / 32x32 block at (x, y)                                              DESIGN 4.16
 *   X265AMD_CHAIN_VERIFY    present | 2    the host repeats what the device's chains decided and fails on a difference (2: merge check, search, RD as well)  DESIGN 4.18
 *   X265AMD_PUB_LOG         present        row publications and the gate's waits for them (dbg/rows_of.py)                                                   DESIGN 4.13
 *   X265AMD_DUMP_CTU        directory      per call: every CTU's input state and outputs, without queues (dbg/vs_dump.py, dbg/ctu_replay.py)                 dbg/README.md
 *   X265AMD_DUMP_POC        integer        per call: the one picture to dump
 *   X265AMD_DUMP_MARGIN     mx,my          per call: how much of the reference pictures around the CTU goes into the dump (horizontal, vertical)
 *   X265AMD_RC_DUMP         path           per picture: its rate-control record in the layout of oracle/ref_rc_dump.cpp, appended (dbg/rc_compare.py)       DESIGN 8
 *   X265AMD_RC_LOG          present        a line per picture with its type, QP and cost                                                                     DESIGN 4.27
 *   X265AMD_WP_DEBUG        letters        s / l / p leave out weighted prediction's picture sums / the lookahead's analysis / the slice's                   DESIGN 4.24
 *   X265AMD_WP_LOG          present        per picture: a weighted slice's weights as the reference's --log-level full prints them                           DESIGN 4.24
 *   X265AMD_WP_FLOOD        mode,groups    per call: a flood of one-wave workgroups in front of every weight-cost launch (a test's load generator)           DESIGN 8
 *   X265AMD_IMPORT_WAIT_S   integer (300)  seconds a picture coded by another encoder object is waited for before the encode fails                           DESIGN 6
 *
 * The host's resources.
 *   X265AMD_QUEUES          integer (224)  device job queues (0: none, every command is a kernel launch on a stream -- pinned by tests/test_device_queue.py)  DESIGN 4.6
 *   X265AMD_WORKERS         integer        the row tasks' worker threads (default: the CPUs this process may use, minus two)                                 DESIGN 4.7
 *   X265AMD_FRAME_THREADS   integer        per encoder: pictures in flight                                                                                   DESIGN 4.8
 *   X265AMD_ROW_THREADS     integer (64)   per call: CTU rows of a picture in flight                                                                         DESIGN 4.7
 *
 * Path selectors: how a stream mismatch is localised.  The other side of each is the general path that other configurations take anyway, and is pinned to the
 * reference's stream like the default (tests/test_device_queue.py; CHAIN_64 by tests/test_encoder_full_size.py).  FILTER_COLS is read for pictures coded in parallel
 * only (frameNumThreads > 1).
 *   X265AMD_CHAIN_64        0 | 1 (0)      the 64x64 CU's levels decided inside the skip chain                                                               DESIGN 4.30
 *   X265AMD_INTRA_CHAIN     1 | 0 (1)      the 8x8 CUs of an I picture's 16x16 block as a chain the device runs (0: one by one through the host)             DESIGN 4.16
 *   X265AMD_INTER_CHAIN     1 | 0 (1)      a P / B CTU's skipped CUs decided by the device's skip chain (0: every CU through the host)                       DESIGN 4.18
 *   X265AMD_FUSED_SEARCH    1 | 0 (1)      a P picture's 2Nx2N search as one command (0: as separate commands)                                               DESIGN 4.19
 *   X265AMD_SEARCH_AHEAD    bits (3)       searches started beside (bit 0: leaves) or behind (bit 1: CUs with sub-CUs) their CU's merge check                DESIGN 4.19
 *   X265AMD_DEVICE_RDOQ     1 | 0 (1)      with RDOQ: the fused intra commands and the intra chain (0: scan and chains apart, the host's bit estimates)      DESIGN 4.23
 *   X265AMD_FILTER_COLS     1 | 0 (1)      in-loop filters and publication by CTU columns behind the analysis (0: by whole rows)                             DESIGN 4.13
 */
#ifndef X265AMD_XA_ENV_H
#define X265AMD_XA_ENV_H
#include <stdlib.h>

/* a string, or nullptr: getenv("X265AMD_...") */
static inline const char* xa_env_str(const char* name) { return getenv(name); }
/* set at all */
static inline bool xa_env_present(const char* name) { return getenv(name) != nullptr; }
/* on unless set to 0 */
static inline bool xa_env_on(const char* name) { const char* v = getenv(name); return !(v && atoi(v) == 0); }
/* off unless set to a non-zero number */
static inline bool xa_env_nonzero(const char* name) { const char* v = getenv(name); return v && atoi(v) != 0; }
/* an integer, d when unset */
static inline int xa_env_int(const char* name, int d) { const char* v = getenv(name); return v ? atoi(v) : d; }
#endif
