/* C ABI of mobgt_amd/libmobgt_checkins.so -- check-in SESSIONS from a raw check-in log, on the device.
 *
 * The reference makes its sessions offline with Python dict loops over every check-in (graphormer/foursquare_process.py):
 * load_trajectory_from_tweets and filter_users_by_length (:115-260) count, filter and cut each user's visits into sessions by
 * time gaps, build_users_locations_dict (:262-294) numbers users, POIs and categories, prepare_neural_data (:377-482) writes the
 * dense rows and splits train from test.  This library is that rule for a log of N records (user, poi, cat, t) in log order,
 * as six entry points; between them the caller runs torch.sort and torch.cumsum (mobgt_amd/checkins.py, whose docstring states
 * the rule; sessionize_host there is the same rule as a plain loop).
 *
 * Ids are dense: users 1 .. U0, POIs 1 .. P0, categories 1 .. C0 (data.first_seen_ids of the raw ids); t is int64 seconds of the
 * local wall clock.  Every count is an integer atomic or a plain store: the results are exact and independent of the order of
 * execution.  Nothing of size U0 x anything or P0 x P0 exists: every buffer is linear in N, U0, P0 or C0.
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  Plain launches on
 * `stream` (the last argument): no allocation, no host synchronisation, no workgroup waits for another.  Buffers are caller-owned
 * device memory, C-contiguous.  Return: 0 on success, one of the MOBGT_CHECKINS_E* codes (checked before anything is launched),
 * or a positive hipError_t of a launch.  EVERY element of every output is written by every call: the caller never pre-zeroes
 * anything.  A pointer to a buffer of zero elements may be null.  An index read from a buffer is checked against the size of
 * what it indexes before it is used; what fails is skipped.
 */
#ifndef MOBGT_CHECKINS_H
#define MOBGT_CHECKINS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_CHECKINS_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_CHECKINS_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */

/* limits of the raw id spaces (2^28; buffers are linear in them, and Gowalla has about 1.3 M venues) */
#define MOBGT_CHECKINS_MAX_U0 268435456
#define MOBGT_CHECKINS_MAX_P0 268435456
#define MOBGT_CHECKINS_MAX_C0 268435456

/* The cut keeps a map of the session length 1 .. session_max + 1 onto itself in the 16 nibbles of one 64-bit word. */
#define MOBGT_CHECKINS_MAX_SESSION_MAX 15

/* records one wave of mobgt_checkins_cut takes per step */
#define MOBGT_CHECKINS_WAVE 64

/* a key of mobgt_checkins_keys for a record that does not remain: sorts behind every real key (INT64_MAX) */
#define MOBGT_CHECKINS_NOKEY 9223372036854775807

/* bits of status[0] */
#define MOBGT_CHECKINS_SBADUSER 1     /* mobgt_checkins_count: a user id outside 1 .. U0                     */
#define MOBGT_CHECKINS_SBADPOI 2      /* mobgt_checkins_count: a POI id outside 1 .. P0                      */
#define MOBGT_CHECKINS_SBADCAT 4      /* mobgt_checkins_count: a category id outside 1 .. C0                 */
#define MOBGT_CHECKINS_SBADINDEX 8    /* any later entry point: an index read from a buffer was out of range */
#define MOBGT_CHECKINS_SZEROSPLIT 16  /* mobgt_checkins_sessions: a surviving user with no train session     */

#define MOBGT_CHECKINS_ABI_VERSION 1
int mobgt_checkins_abi_version(void);

/* Step 1 of the rule (:161-187): records per user and per POI over the whole log, and every user's sort key.
 *
 * In:  user, poi, cat [N] int32   the log
 * Out: ucnt [U0] int32    records of user u (ucnt[u - 1])
 *      pcnt [P0] int32    records at POI p
 *      ufirst [U0] int32  the log position of the user's first record; INT32_MAX for a user without one
 *      ukey [U0] int64    (INT32_MAX - ucnt) << 32 | ufirst where ucnt >= trace_min, else MOBGT_CHECKINS_NOKEY: ascending keys
 *                         are the kept users by count descending, ties by first appearance (:185, a stable sort over dict order)
 *      status [1] int32   0, or SBADUSER / SBADPOI / SBADCAT bits
 * A record with ANY id outside its range is skipped whole -- it is counted nowhere, and mobgt_checkins_keys skips it again --
 * and its bits are raised.  Three launches: a fill, one thread per record (global integer atomics), one thread per user.
 * Limits: 0 <= N < 2^31, 1 <= U0 / P0 / C0 <= their MAX, trace_min >= 0 -- else EBADDIM. */
int mobgt_checkins_count(const void* user, const void* poi, const void* cat, int64_t N, int64_t U0, int64_t P0, int64_t C0,
                         int64_t trace_min, void* ucnt, void* pcnt, void* ufirst, void* ukey, void* status, void* stream);

/* The key of every record: which user it belongs to (by rank) and where it stands in the log.
 *
 * In:  urank [U0] int32   the rank of user u among the kept users (0 .. U1 - 1, from the sorted ukey), -1 for a user not kept
 *      pcnt [P0] int32    mobgt_checkins_count's
 * Out: keys [N] int64     (rank << 32) | i for a record that REMAINS: ids in range, its user kept, pcnt of its POI >=
 *                         global_visit (:186, :211-214); else MOBGT_CHECKINS_NOKEY
 * One launch, one thread per record.  Sorted ascending, the keys below NOKEY are the remaining records, user after user in the
 * order of step 1, each user's in log order.  Limits as above, global_visit >= 0, 0 <= U1 <= U0. */
int mobgt_checkins_keys(const void* user, const void* poi, const void* cat, int64_t N, int64_t U0, int64_t P0, int64_t C0,
                        const void* urank, int64_t U1, const void* pcnt, int64_t global_visit, void* keys, void* stream);

/* Step 2, the cut (:197-246).
 *
 * In:  keys [R] int64   the R remaining records' keys, ascending
 *      t [N] int64      the log's times
 * Out: start [R] int32  1 where record j starts a session, else 0
 *      member [R] int32 1 where record j is in a session (it starts one or is appended), 0 where it is dropped
 *      status [1] int32 SBADINDEX is OR-ed in (not reset) where a key's log position is outside 0 .. N - 1
 * With g = t - t of the user's previous remaining record and s the length of the user's current session: the first record
 * starts; else g >= hour_gap_s or s > session_max starts; else g >= min_gap_s appends; else the record is dropped.
 *
 * One launch, ONE WAVE PER USER (four users per workgroup): the wave finds its user's segment by two binary searches in the
 * keys and walks it MOBGT_CHECKINS_WAVE records at a time with coalesced loads.  A lane takes the previous record's t from its
 * neighbour by shuffle, lane 0 from the chunk before.  Each record is a map of s in 1 .. session_max + 1 onto itself -- RESET
 * (s -> 1), APPEND (s -> s + 1; -> 1 where s > session_max), SKIP (s -> s; -> 1 where s > session_max) -- kept as 16 nibbles
 * of a 64-bit word; maps compose, so an inclusive scan of composed maps over the wave (six shuffle steps), applied to the state
 * carried in from the chunk before, gives every record the state before it, which decides its action.
 * A record is written by the wave of its key's rank: every element of start and member is written given that every rank is
 * below U1, which mobgt_checkins_keys guarantees.
 * Limits: 0 <= R <= N < 2^31, 0 <= U1, 1 <= session_max <= MOBGT_CHECKINS_MAX_SESSION_MAX, 0 <= min_gap_s, hour_gap_s. */
int mobgt_checkins_cut(const void* keys, int64_t R, const void* t, int64_t N, int64_t U1, int64_t hour_gap_s, int64_t min_gap_s,
                       int session_max, void* start, void* member, void* status, void* stream);

/* Step 3 (:249-259) and the train split (:433-435): which sessions and users survive.
 *
 * In:  keys, start, member [R]   as above
 *      scum [R] int64            the inclusive prefix sum of start: scum[j] - 1 is the raw session of record j; S0 = scum[R - 1]
 * Out: slen [S0] int32     members of raw session s
 *      suser [S0] int32    its user's rank
 *      ukept [U1] int32    the user's sessions with slen >= session_min
 *      sfinal [S0] int32   1 where slen >= session_min and the user has ukept >= sessions_min, else 0
 *      outlen [S0] int32   slen where sfinal, else 0
 *      usurv [U1] int32    1 where ukept >= sessions_min
 *      ukept_s [U1] int32  ukept where usurv, else 0
 *      split [U1] int32    (int)floor(train_split * (double)ukept) in float64, 0 where not usurv
 *      emit [R] int32      1 where record j is an output check-in: member and sfinal of its session
 *      status [1] int32    SBADINDEX / SZEROSPLIT are OR-ed in (not reset)
 * Five launches: a fill, the records (integer atomics into slen; the starting record stores suser), the sessions (integer atomics
 * into ukept), the selection (sessions and users), the records again (emit).
 * Limits: 0 <= S0 <= R < 2^31, 0 <= U1, session_min >= 0, sessions_min >= 0, 0 < train_split <= 1. */
int mobgt_checkins_sessions(const void* keys, const void* start, const void* member, const void* scum, int64_t R, int64_t S0,
                            int64_t U1, int64_t session_min, int64_t sessions_min, double train_split, void* slen, void* suser,
                            void* ukept, void* sfinal, void* outlen, void* usurv, void* ukept_s, void* split, void* emit,
                            void* status, void* stream);

/* Step 4, first half: the log position of every output check-in and where every POI and category first appears in the output.
 *
 * In:  keys, emit [R]; ocum [R] int64  the inclusive prefix sum of emit: ocum[j] - 1 is the output position of record j, M = ocum[R - 1]
 *      poi, cat [N] int32              the log
 * Out: kept [M] int64     the log position of output check-in o
 *      pfirst [P0] int32  the first output position of POI p, INT32_MAX for a POI not in the output (integer atomic min)
 *      cfirst [C0] int32  the same for the check-ins' own categories
 *      pflag, cflag [M] int32   1 where output check-in o is the first of its POI / of its category
 *      status [1] int32   SBADINDEX is OR-ed in (not reset)
 * Three launches: a fill (kept too: -1), the records, the output check-ins.  Limits: 0 <= M <= R <= N < 2^31. */
int mobgt_checkins_first(const void* keys, const void* emit, const void* ocum, int64_t R, int64_t M, const void* poi, const void* cat,
                         int64_t N, int64_t P0, int64_t C0, void* kept, void* pfirst, void* cfirst, void* pflag, void* cflag,
                         void* status, void* stream);

/* Step 4, second half, and the packed dataset.
 *
 * In:  kept, pflag, cflag [M]; pfirst [P0], cfirst [C0]; poi, cat [N] int32, t [N] int64
 *      pnum, cnum [M] int64    the inclusive prefix sums of pflag / cflag: at a first appearance, the new id (P, n_cat: the last)
 *      sfinal, suser [S0] int32; scum2, lcum [S0] int64   the inclusive prefix sums of sfinal (S: the last) and outlen (M)
 *      ucum, kcum [U1] int64   the inclusive prefix sums of usurv (U) and ukept_s (S); ukept_s, split [U1] int32
 * Out: seq [M, 3] int32      rows (new POI id, time slot = (t mod 86400) div 1800 with a floor mod, the new id of the FIRST-SEEN
 *                            category of the row's POI: of the category of check-in pfirst[poi], :293-294, :425)
 *      poi_log [P] int32     the log position of the first output check-in of new POI id k + 1 (raw id, coordinates: :279)
 *      cat_log [n_cat] int32 the same for the categories
 *      offsets [S + 1] int64, users [S] int64 (new user ids 0 .. U - 1), train [S] uint8 (the user's first `split` sessions)
 *      n, mult [S] int32     distinct POIs of the session's history (all rows but the last) and the largest multiplicity there
 *      user_log [U] int32    the rank (0 .. U1 - 1) of new user id k
 *      status [1] int32      SBADINDEX is OR-ed in (not reset)
 * Four launches: a fill (every output; offsets[0] = 0), the output check-ins, the sessions and users, the sessions again (n and
 * mult read the finished seq; a session has at most session_max + 1 <= 16 rows).
 * Limits: 0 <= M <= N < 2^31, 0 <= P <= M, 0 <= n_cat <= M, 0 <= S <= S0, 0 <= U <= U1. */
int mobgt_checkins_emit(const void* kept, const void* pflag, const void* cflag, const void* pnum, const void* cnum, int64_t M,
                        const void* pfirst, const void* cfirst, const void* poi, const void* cat, const void* t, int64_t N, int64_t P0,
                        int64_t C0, int64_t P, int64_t n_cat, const void* sfinal, const void* suser, const void* scum2,
                        const void* lcum, int64_t S0, int64_t S, const void* ucum, const void* kcum, const void* ukept_s,
                        const void* split, int64_t U1, int64_t U, void* seq, void* poi_log, void* cat_log, void* offsets, void* users,
                        void* train, void* n, void* mult, void* user_log, void* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
