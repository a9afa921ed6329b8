/* rmpc_cbs.h -- optimal timed routes for a fleet: conflict-based search (CBS; Sharon, Stern, Felner,
 * Sturtevant 2015) over the cells, layers, sep2 / lag conflicts and single-robot route search of
 * rmpc_timed_plan_device.  A header of its own beside rmpc.h, whose entries are what they were and whose words -- cell,
 * CONFLICT, d2, reach, rules 1 to 7, status, arrive -- are used here as they stand there.  Written in the forms
 * robot_mpcs_amd/_abi.py reads.
 *
 * PROBLEM.  What rmpc_timed_plan_device takes, without orders: grid [H][W], occ_threshold, movement, B robots with
 * start_cell [B] and goal_index [B] into fields [Gf][H][W] / goal_cells [Gf], the window T, sep2 and lag.
 *
 * SKIPPED.  A robot skipped by rule 1 has path -1, status RMPC_GRID_OUTSIDE and arrive T + 1.  It is in no conflict and is
 * never constrained.
 *
 * ROUTE UNDER A TABLE.  A constraint table C is a set of (t, cell) with t >= 1.  The route of robot b under C is rules 2
 * to 7 of rmpc_timed_plan_device with res[t] replaced by C[t], no later-starts rule and nothing stamped; if some layer
 * reach[t] is empty the route DOES NOT EXIST.  Otherwise te = T, the status is 0, and the route's arrive is the least
 * arrival any path under C can have.  For a path under C lies in reach[t] at every t, and one that holds the goal g from
 * layer a' on has g in reach[a' .. T].  If reach[T] holds g, then g is its least (D, c), D(g) = 0 being the field's only
 * zero; the backtrack waits first, so it stays on g down to the least a with g in reach[a .. T], and a <= a'.  If reach[T]
 * does not hold g, no path under C ends on it and every one has arrive T + 1, as the route has.
 *
 * CONFLICT.  Robots i < j, neither skipped, and layers t of i and s of j with |t - s| <= lag and (t, s) != (0, 0)
 * conflict when d2(p_i[t], p_j[s]) < sep2.  A node's conflict is the least by (min(t, s), i, j, t, s).
 *
 * NODE.  A node has a parent and one constraint; a path and an arrive per robot; cost = the sum of arrive (a skipped
 * robot counts T + 1); and its conflict, or none: a node with no conflict is a SOLUTION.  Node 0 has no constraint and
 * every robot's route under the empty table; it is dead when one of them does not exist.  A robot's table in a node is
 * the union of the constraints on that robot along the chain to the root.
 *
 * CHILDREN of a node with conflict (i, t, j, s), v = p_j[s]:
 *  child 0 exists when t >= 1: robot i keeps clear of v around s -- every cell that conflicts with v, in every layer u
 *          with |u - s| <= lag and 1 <= u <= T, joins i's table;
 *  child 1 exists when s >= 1: (s, v) joins j's table.
 * In a child only the constrained robot is re-routed; a child whose route does not exist is dead.
 * SOUND: a set of paths that breaks both constraints has i inside v's disc within lag of s while j stands on v at s,
 * which is a conflict; so every conflict-free set of paths under the parent's tables lives under one of the two
 * children.  When t = 0 robot i stands on its start whatever it is told, so every conflict-free set has j off v at s:
 * child 1 alone holds them all; likewise child 0 alone when s = 0.  PROGRESS: each child excludes the parent's own paths
 * (child 0 the cell p_i[t], which conflicts with v within lag of s; child 1 the cell v at s).  A child's table contains
 * its parent's, so by ROUTE UNDER A TABLE its cost is never below its parent's.
 *
 * IDS.  Expansions are numbered x = 0, 1, ... in the order they are taken; the children of expansion x get the ids
 * 1 + 2 x and 2 + 2 x.  A missing or dead child leaves its id unused.
 *
 * ROUND.  A node is OPEN when it has been created, is not dead, is not a solution and has not been expanded.  The
 * incumbent is the solution with the least (cost, id); Lo is the least cost among the open nodes, +inf without one.  Open
 * nodes whose cost is not below the incumbent's are never taken.  One round:
 *  1. if there is an incumbent and incumbent.cost <= Lo: outcome RMPC_CBS_SOLVED, stop;
 *  2. if nothing is open and there is no incumbent: RMPC_CBS_INFEASIBLE, stop;
 *  3. take the e <= expand takeable open nodes that are least by (cost, id); if their children's ids would reach
 *     `nodes` (2 (expanded + e) >= nodes): RMPC_CBS_POOL, stop, and take none; otherwise expand them in that order and
 *     add 1 to rounds_run.
 * After `rounds` rounds of a call without a stop the outcome is RMPC_CBS_ROUNDS.
 *
 * RESUME.  With resume != 0 and the same arguments a call continues the search whose state the workspace holds (after
 * ROUNDS for `rounds` more; after POOL it stops again at once, the pool being what it was): `rounds` rounds in one call
 * and in slices give the same result in every bit.  A workspace that holds no search of these arguments is answered with
 * RMPC_CBS_BAD_STATE and the outputs of a search without nodes.
 *
 * OUTPUTS.  info [RMPC_CBS_INFO] int32: [RMPC_CBS_OUTCOME]; [RMPC_CBS_NODE] the incumbent, else the open node least by
 * (cost, id), else -1; [RMPC_CBS_CONFLICT_FREE] 1 when that node is a solution; [RMPC_CBS_COST] its cost;
 * [RMPC_CBS_BOUND] min(Lo, incumbent.cost) at the stop; [RMPC_CBS_CREATED] the nodes created (dead ones are not);
 * [RMPC_CBS_EXPANDED]; [RMPC_CBS_ROUNDS_RUN] over all slices.  paths [B][T + 1], status [B] (0 or RMPC_GRID_OUTSIDE) and
 * arrive [B] are that node's.  Without a node: paths -1, arrive T + 1, status as a skipped robot's or 0, cost
 * RMPC_CBS_INF.  A bound of +inf is RMPC_CBS_INF.
 *
 * IT FOLLOWS that
 *  (a) with RMPC_CBS_SOLVED no conflict-free set of paths of the window has a smaller sum of arrive: every such set
 *      lives under an open node or a solution (SOUND), whose cost is a lower bound on it (ROUTE UNDER A TABLE, robot by
 *      robot), and every one of those costs is >= the incumbent's;
 *  (b) bound never falls from slice to slice: a taken node is replaced by children of no lower cost;
 *  (c) every failure-free order of rmpc_timed_plan_device on the same problem (all status <= 0) is a conflict-free set of
 *      paths in these moves, so its sum of arrive is >= bound, and >= cost when solved;
 *  (d) a reported node with conflict_free meets the GUARANTEE of rmpc_timed_plan_device for every pair, so
 *      rmpc_timed_follow_device takes its paths unchanged;
 *  (e) with B = 1, or with no conflict at the root, the result is the root with rounds_run 0.
 * Everything is integer work on cells except the ranking of end cells: every result is bitwise the same on every run.
 *
 * The host enqueues the root, `rounds` rounds and the report blind; no workgroup waits for another; every kernel behind
 * a stop returns at once on a flag in the workspace.  No host reads, no synchronisation, no allocation; takes a stream,
 * needs no handle, runs on the device of grid.
 * work: rmpc_cbs_work_bytes(H, W, T, B, nodes, expand) bytes (-1 for sizes that are refused), contents irrelevant unless
 * resume != 0.  Refused before any HIP call (-1, rmpc_last_error): a struct_size other than sizeof(rmpc_cbs), NULL
 * pointers, what rmpc_timed_plan_device refuses of H, W, movement, T, sep2, lag and Gf, B outside
 * [1, RMPC_CBS_MAX_ROBOTS], nodes outside [1, RMPC_CBS_MAX_NODES], expand outside [1, RMPC_CBS_MAX_EXPAND], rounds
 * outside [0, RMPC_CBS_MAX_ROUNDS], a workspace that is too small. */
#ifndef RMPC_CBS_H
#define RMPC_CBS_H

#include <stdint.h>

#include "rmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_CBS_MAX_ROBOTS 64
#define RMPC_CBS_MAX_NODES 1048576
#define RMPC_CBS_MAX_EXPAND 256
#define RMPC_CBS_MAX_ROUNDS 4096

#define RMPC_CBS_SOLVED 1
#define RMPC_CBS_INFEASIBLE 2
#define RMPC_CBS_POOL 3
#define RMPC_CBS_ROUNDS 4
#define RMPC_CBS_BAD_STATE 5

#define RMPC_CBS_INF 2147483647

#define RMPC_CBS_INFO 8
#define RMPC_CBS_OUTCOME 0
#define RMPC_CBS_NODE 1
#define RMPC_CBS_CONFLICT_FREE 2
#define RMPC_CBS_COST 3
#define RMPC_CBS_BOUND 4
#define RMPC_CBS_CREATED 5
#define RMPC_CBS_EXPANDED 6
#define RMPC_CBS_ROUNDS_RUN 7

typedef struct rmpc_cbs {
  int32_t struct_size;                 /* sizeof(rmpc_cbs) */
  int32_t H, W, movement;
  const double *grid;                  /* [H][W] */
  double occ_threshold;
  int32_t B, Gf;
  const int32_t *start_cell;           /* [B] */
  const int32_t *goal_index;           /* [B] into fields / goal_cells */
  const double *fields;                /* [Gf][H][W] */
  const int32_t *goal_cells;           /* [Gf] */
  int32_t T, sep2, lag;
  int32_t nodes, expand, rounds;       /* pool capacity M, nodes taken per round E, rounds of this call R */
  int32_t resume;                      /* 0: a new search; otherwise continue the one the workspace holds */
  void *work; int64_t work_bytes;      /* rmpc_cbs_work_bytes(H, W, T, B, nodes, expand) */
  int32_t *paths, *status, *arrive;    /* [B][T + 1], [B], [B] out */
  int32_t *info;                       /* [RMPC_CBS_INFO] out */
} rmpc_cbs;

int64_t rmpc_cbs_work_bytes(int H, int W, int T, int B, int nodes, int expand);
int rmpc_cbs_device(const rmpc_cbs *p, void *stream);

#ifdef __cplusplus
}
#endif

#endif
