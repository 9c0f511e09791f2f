/* C ABI of mobgt_amd/libmobgt_prefixes.so -- every PREFIX of a check-in session as a sample, on the device.
 *
 * The reference makes one sample of a session (gen_pickles.py:760-761: hist_traj = all_traj[:-1], target = all_traj[-1]); its own
 * Markov baseline scores every step of every session (graphormer/train.py:436-446).  This library lists the samples of the second
 * protocol and gives each the two numbers the data path needs before it looks at a sample (mobgt_amd/prefixes.py, whose docstring
 * states the rule; prefix_stats_host there is the same rule as a plain loop).
 *
 * A session has rows r_0 .. r_L, L >= 1: offsets[s + 1] - offsets[s] = L + 1 rows of seq.  For min_history = h it yields the
 * samples c = h .. L: sample c has history r_0 .. r_{c-1} and target r_c.  With occ_j = the number of i <= j with poi_i == poi_j:
 *
 *     n_c    = #{j < c : occ_j == 1}    distinct POIs of the history
 *     mult_c = max_{j < c} occ_j        the largest multiplicity of a POI there
 *
 * an inclusive sum-scan and an inclusive max-scan along the session.  Integers: every result is exact.
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  Plain launches on
 * `stream` (the last argument): no allocation, no host synchronisation, no workgroup waits for another.  Buffers are caller-owned
 * device memory, C-contiguous.  Return: 0 on success, one of the MOBGT_PREFIXES_E* codes (checked before anything is launched),
 * or a positive hipError_t of a launch.  EVERY element of every output is written by every call: the caller never pre-zeroes
 * anything.  A pointer to a buffer of zero elements may be null.  An index read from a buffer is checked against the size of
 * what it indexes before it is used; what fails is skipped.
 */
#ifndef MOBGT_PREFIXES_H
#define MOBGT_PREFIXES_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_PREFIXES_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_PREFIXES_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */

/* history rows of one session (= MOBGT_DATA_MAX_LP: the collator converts longer histories on the host); its POI column is
 * staged in 16 KB of LDS */
#define MOBGT_PREFIXES_MAX_L 4096

/* history rows one wave takes per step; a session of at most this many takes the form without LDS */
#define MOBGT_PREFIXES_WAVE 64

/* bits of status[0]; a session that raises one is skipped */
#define MOBGT_PREFIXES_SBADINDEX 1    /* offsets or pcum entries out of range, descending, or not the sample count */
#define MOBGT_PREFIXES_STOOLONG 2     /* a session that yields samples has more than MAX_L history rows            */

#define MOBGT_PREFIXES_ABI_VERSION 1
int mobgt_prefixes_abi_version(void);

/* The samples of S sessions and their n and mult.
 *
 * In:  seq [M, 3] int32      rows (poi, time slot, category); only the POI column is read, any int32 is an id
 *      offsets [S + 1] int64 session s is rows offsets[s] .. offsets[s + 1] - 1
 *      pcum [S + 1] int64    the output position of session s's first sample; pcum[S] = Q
 *      keep [S] uint8        or NULL (every session): a session with keep[s] == 0 yields nothing
 * Out: session [Q] int32     the session of sample q: session-major, c ascending inside a session
 *      cut [Q] int32         its c: the sample is rows 0 .. c of its session, the last of them the target
 *      n, mult [Q] int32     as above
 *      status [1] int32      0, or SBADINDEX / STOOLONG bits
 * The sample count of session s is L - min_history + 1 where it is kept and L >= min_history, else 0.  Before anything of a
 * session is used, its four entries are checked: 0 <= offsets[s] <= offsets[s + 1] <= M, 0 <= pcum[s] <= pcum[s + 1] <= Q and
 * pcum[s + 1] - pcum[s] == the sample count.  A session that fails is skipped and SBADINDEX is raised; the samples of a skipped
 * session keep what the fill wrote: session -1, cut / n / mult 0.
 *
 * Three launches.  A fill of every output.  The short form, ONE WAVE PER SESSION (four sessions per workgroup) for L <=
 * MOBGT_PREFIXES_WAVE: lane j holds poi_j, counts occ_j over L broadcasts by shuffle, the two scans take six shuffle steps each,
 * lanes h - 1 .. L - 1 store their sample; no LDS.  The long form for L > MOBGT_PREFIXES_WAVE, one wave per workgroup: the waves
 * look through the sessions 64 at a time, and for each long one stage its POI column in LDS, walk it 64 rows at a time -- a lane
 * counts the matches among the rows of the chunks before with broadcast 16-byte LDS reads, among its own chunk's by shuffle --
 * and carry (n, mult) from one chunk into the next.
 * Limits: 0 <= S < 2^31, 0 <= Q <= M < 2^31, 1 <= min_history -- else EBADDIM. */
int mobgt_prefixes_stats(const void* seq, const void* offsets, const void* pcum, const void* keep, int64_t S, int64_t M, int64_t Q,
                         int64_t min_history, void* session, void* cut, void* n, void* mult, void* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
