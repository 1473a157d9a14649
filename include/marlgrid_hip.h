/*
 * marlgrid_hip.h — C ABI of the MI355X-native batched MarlGrid step engine
 * (libmarlgrid_hip.so, built from marlgrid_amd/csrc by hipcc --offload-arch=gfx950).
 *
 * The reference (kandouss/marlgrid v0.0.5) is pure Python with no FFI; the boundary this library
 * sits behind is the Python class contract of `MultiGridEnv` (marlgrid/base.py:334-708).  Each
 * entry point below names the reference method(s) it replaces for a BATCH of B independent envs:
 *
 *   mg_mt_seed      MultiGridEnv.seed -> gym.utils.seeding.np_random -> RandomState.seed(list)
 *                                                                       (base.py:371-374)
 *   mg_reset        MultiGridEnv.reset + _gen_grid + place_obj/try_place_obj
 *                                       (base.py:402-416, 664-708; envs/empty.py:9-16,
 *                                        envs/cluttered.py:25-36, envs/goalcycle.py:30-51)
 *   mg_step         MultiGridEnv.step action loop, rewards, done  (base.py:501-649); with a reset
 *                   program also the reset() of every env whose episode just ended (auto-reset)
 *   mg_step_render  the two above + mg_render_obs in one launch: the whole MultiGridEnv.step (base.py:501-653)
 *   mg_render_obs   MultiGridEnv.gen_obs / gen_agent_obs / gen_obs_grid, MultiGrid.slice,
 *                   MultiGrid.opacity, GridAgentInterface.process_vis / occlude_mask,
 *                   MultiGrid.render / render_tile / blend_tiles
 *                                       (base.py:418-474, 123-147, 103-106, 275-331;
 *                                        agents.py:233-266, 290-343)
 *   mg_encode       MultiGrid.encode    (base.py:196-214; objects.py:90-99)
 *   mg_encode_views every agent's gen_obs_grid(agent) -> grid.encode(vis_mask) (base.py:418-451, 196-214)
 *   mg_step_encode_views  mg_step + mg_encode_views: MultiGridEnv.step with encoded views instead of pixels
 *   mg_step_ep / mg_step_render_ep / mg_step_encode_views_ep   the three steps above with an MgEpisode: next-step auto-reset
 *                   (the terminal state is returned, the env's next call is its reset) and the episode's flags, length and
 *                   return from the step's own launch (base.py:512, 576-581, 627-649)
 *   mg_step_render_delta / mg_step_render_delta_ex   mg_step_render (_ex: with the encode and / or an MgEpisode) that does not
 *                   store again the observation bands its output buffer already holds
 *   mg_goal_distance  (no reference counterpart: the exact number of left / right / forward actions from every agent, or every
 *                   state, to the step that enters a goal cell; -1 where there is no path)
 *   mg_solve_distance (none either: the same through keys and doors — left / right / forward / pickup / toggle —, with the
 *                   first action of a shortest path)
 *   mg_fork_rows / mg_rollout  (none either: rows of the batch copied into a shadow state and stepped T times there — what T
 *                   MultiGridEnv.step calls WOULD return, the env untouched)
 *   mg_explore_update  (none either: per agent, the world cells its observations have covered this episode and how often it
 *                   stood on each cell — what count-based exploration bonuses are made of)
 *   mg_memory_update   (none either: mg_explore_update, and per agent what each cell showed when it was last seen, and when)
 *   mg_put_obj      MultiGridEnv.put_obj (base.py:655-662)
 *   mg_place        MultiGridEnv.place_obj / try_place_obj outside _gen_grid (base.py:664-708)
 *   mg_render_frame MultiGridEnv.render's whole-grid image: MultiGrid.render(top_agent=None) +
 *                   visibility highlight         (base.py:714-759, 301-331)
 *   mg_render_kernel_name  (no reference counterpart: names the launch for profiles and warns of generic instantiations)
 *   mg_render_specialize   (none either: compiles, at run time, the instantiation of the observation kernel a (view_size,
 *                   tile_size) pair off the library's table would have; mg_step_render_spec / mg_render_obs_spec launch it)
 *   mg_obs_place    the observation arrays MultiGridEnv's constructor / gen_obs allocate (base.py:334-347, 453-474),
 *                   for a batch: where in HBM they lie (construction time; mg_obs_release, mg_obs_trim)
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every buffer is owned by the
 * caller and lives in device memory (HBM) unless marked HOST; kernels never allocate.  All calls
 * are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream) and
 * return 0 or a negative MG_E_* code for argument errors detected on the host.  Per-env runtime
 * errors (the reference's exceptions) are recorded in MgState.error[b] (first error sticks) and
 * surfaced by the host wrapper as the matching Python exception.  Re-entrant: no mutable globals (the one
 * exception, behind a mutex: the record of placed observation buffers, mg_obs_place below).
 *
 * HBM layout (struct-of-arrays over the env batch, sized for 288 GB):
 *   grid        uint8  [B][cells_stride]      object id per cell, index x*H + y (= MultiGrid.grid[i,j]);
 *                                            cells_stride = W*H rounded up to 16
 *   agents      uint64 [B][n_agents]          packed record, see MG_AG_* below
 *   mt          uint32 [B][624] + mt_pos[B]   per-env MT19937 (numpy RandomState stream), *lazy*
 *                                            form: word mt_pos is the next one to regenerate
 *   mt_head     uint32 [B][16]                the 16 outputs generated last and not consumed yet
 *                                            (tempered), contiguous per env: what a step draws from
 *   step_count  int32  [B];  done uint8 [B];  error int32 [B]
 *   error_flag  int32  [1]  HOST-mapped (mg_host_flag_alloc) or device: becomes non-zero when any
 *                                            error[b] is set — a host polls this one word instead of
 *                                            scanning error[B] after every launch
 *   obs         uint8  [B][n_agents][P][P][3] with P = view_size*tile_size
 */
#ifndef MARLGRID_HIP_H
#define MARLGRID_HIP_H

#if !defined(__HIPCC_RTC__)   /* (hipRTC has no system headers: the source that includes this file supplies the types) */
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MG_ABI_VERSION 6
#define MG_MAX_AGENTS 32  /* agents per env (the reference: any number, base.py:335-369; register_marl_env asserts <= 6) */
#define MG_MAX_OBJ 256    /* object kinds incl. id 0 = None: the ids are uint8, as the reference's registry keys are (base.py:25,91) */
#define MG_MAX_GEN 1024   /* ops of a reset program (device memory: a sanity bound, not a buffer size) */
/* `_rand_int` draws of a reset program (MgGenOp below) */
#define MG_GEN_DRAWS 8            /* draw registers per program: draw r lives in byte r of one 64-bit scalar during the reset */
#define MG_GEN_SYM 0x40000000     /* an operand x0/y0/x1/y1 with this bit is `const +- draw[r]`, not a plain integer: */
#define MG_GEN_NEG 0x20000000     /*   set: const - draw[r]; clear: const + draw[r] */
#define MG_GEN_DRAW_SHIFT 16      /*   r = (operand >> 16) & 7; const = (int16_t)(operand & 0xFFFF) */
#define MG_GEN_PARAM (-2)         /* MgGenOp.max_tries of a PARAM op: a draw register loaded from the env's row of the parameter table */
#define MG_GEN_EDITS (-3)         /* MgGenOp.max_tries of an EDITS op: the env's own list of cell edits, applied in order */
#define MG_GEN_MAX_EDITS 64       /* entries of an env's edit list, at most (MgGenOp.count of an EDITS op) */
/* the guard of a reset-program op, in the upper bits of MgGenOp.obj (values that were illegal before: ABI 6 still) */
#define MG_GEN_GUARD 0x40000000   /* the op runs only if lo <= draw[r] <= hi (lo <= hi); else it is skipped entirely */
#define MG_GEN_GUARD_DRAW_SHIFT 24 /*   r = (obj >> 24) & 7 */
#define MG_GEN_GUARD_HI_SHIFT 16  /*   hi = (obj >> 16) & 0xFF */
#define MG_GEN_GUARD_LO_SHIFT 8   /*   lo = (obj >> 8) & 0xFF; the low byte keeps its meaning (object id / draw register) */
#define MG_MAX_VIEW 31    /* view_size (agents.py:19-35: any; a view row is a 32-bit mask here) */
#define MG_KEY_WORDS 2
#define MG_MT_N 624
#define MG_MT_HEAD 16

/* host-side argument errors (return values) */
#define MG_OK 0
#define MG_E_ARG (-100)
#define MG_E_UNSUPPORTED (-101)
#define MG_E_LAUNCH (-102)
#define MG_E_NOMEM (-103)   /* mg_obs_place: the device could not hold the buffers */

/* per-env runtime errors (MgState.error), mirroring the reference's exceptions */
#define MG_ERR_VALUE 1     /* ValueError: unknown action               base.py:619-620 */
#define MG_ERR_RECURSION 2 /* RecursionError: rejection sampling failed base.py:705-706 */
#define MG_ERR_TYPE 3      /* TypeError: Box.toggle arity               objects.py:381-382 */
#define MG_ERR_ASSERT 4    /* AssertionError: grid.get out of bounds    base.py:154-156 */
#define MG_ERR_ATTRIBUTE 5 /* AttributeError: None.can_overlap() — an agent whose cell put_obj(None) emptied moves on
                            * (base.py:555-558; see MG_AF_EVICTED) */

/* packed agent record (uint64, little endian bytes) */
#define MG_AG_X 0      /* byte 0: x */
#define MG_AG_Y 1      /* byte 1: y */
#define MG_AG_DIR 2    /* byte 2: dir 0..3 (agent.state % 4, objects.py:132-142); survives reset */
#define MG_AG_FLAGS 3  /* byte 3: MG_AF_* */
#define MG_AG_CARRY 4  /* byte 4: carried object id (0 = None) */
#define MG_AG_RANK 5   /* byte 5: arrival rank among the env's agents (stack order = rank order) */
#define MG_AG_BONUS 6  /* byte 6: bonus_state, 0xFF = None (agents.py:169) */
#define MG_AF_ACTIVE 1
#define MG_AF_DONE 2
#define MG_AF_PLACED 4
#define MG_AF_EVICTED 8 /* put_obj replaced the cell the agent stood on (base.py:655-662: `grid.set` drops whatever was
                         * there): the agent is in no cell any more — nobody sees it, nothing stands on it — but keeps
                         * its position, turns and looks; its next successful forward move raises what upstream's
                         * "remove agent from old cell" raises (base.py:555-559): AssertionError on a solid object,
                         * ValueError (list.remove) on an overlappable one or another agent, AttributeError on None */

/* object descriptor flags */
#define MG_OF_CAN_OVERLAP 1
#define MG_OF_CAN_PICKUP 2
#define MG_OF_SEE_BEHIND 4
#define MG_OF_ENDS_EPISODE 8 /* isinstance(fwd_cell, (Lava, Goal))  base.py:584 */
#define MG_OF_IS_KEY 16
#define MG_OF_IS_DOOR 32
#define MG_OF_IS_BOX 64
#define MG_OF_DOOR_LOCKED 128

/* one entry per object id (id 0 = None); 32 bytes */
typedef struct MgObjDesc {
    uint8_t type_idx, color_idx, state, flags; /* WorldObj.encode + predicates, objects.py:75-99 */
    uint8_t reward_kind;                       /* 0 none, 1 Goal (constant), 2 BonusTile */
    uint8_t toggle_next;                       /* Door closed<->open successor id */
    uint8_t unlock_next;                       /* Door locked->closed successor id */
    uint8_t ovl_slot;                          /* atlas slot for "object + agent on top", 0xFF none */
    uint8_t bonus_id, n_bonus, bonus_flags;    /* bonus_flags: 1 initial_reward, 2 reset_on_mistake */
    uint8_t flags2;                            /* 1: a corner pixel of the plain tile is black (base.py:297) */
    uint32_t pad1;
    double reward;                             /* Goal.reward / BonusTile.reward */
    double penalty;                            /* BonusTile.penalty */
} MgObjDesc;

typedef struct MgConfig {
    int32_t B, W, H, n_agents;
    int32_t view_size, tile_size, view_offset, see_through_walls; /* agents.py:19-35 (uniform) */
    int32_t max_steps, reward_decay, ghost_mode, respawn;         /* base.py:341-346.  ghost_mode bits:
                                                                   * 1 = moves may enter occupied cells (`ghost_mode is
                                                                   * not False`, base.py:541), 2 = placements may land on
                                                                   * occupied cells (`bool(ghost_mode)`, base.py:683) */
    int32_t cells_stride;                                         /* bytes per env in `grid` */
    int32_t n_obj;                                                /* valid object ids: 0..n_obj-1 */
    int32_t n_ovl_slots;                                          /* slot 0 = empty cell */
    int32_t n_tiles;                                              /* >= 1 + n_obj + n_ovl_slots*n_agents*4 */
    int32_t agent_type_idx;                                       /* 13 */
    int32_t atlas_gather_off;                                     /* 0, or the byte offset from `atlas` (a multiple of 16) of a copy of
                                                                   * the atlas in the gather raster's LDS layout — per tile row 16 zero
                                                                   * bytes, its 3 * tile_size bytes, zeros up to a multiple of 4; 32 zero
                                                                   * bytes behind the last row; the whole rounded up to 16 —: the
                                                                   * gather instantiations (mg_render_kernel_name: <.., 2>) then copy it as
                                                                   * it is instead of building it per workgroup (was: reserved) */
    int32_t spawn_x0, spawn_y0, spawn_x1, spawn_y1;               /* agent_spawn_kwargs top / size clamped to the
                                                                   * grid like base.py:692-695: agents are placed
                                                                   * in [x0,x1) x [y0,y1) (base.py:411, 505, 643) */
    int32_t spawn_max_tries;                                      /* agent_spawn_kwargs max_tries, 1..100000 */
    int32_t n_view;                                               /* 0: every agent is rendered with the view
                                                                   * parameters above.  k > 0: only the k agents
                                                                   * view_agent[0..k) are (obs [B][k][P][P][3]) — an env
                                                                   * whose agents differ in view size / tile size /
                                                                   * offset (agents.py:19-35) is rendered group by group,
                                                                   * one mg_render_obs per group with that group's
                                                                   * view parameters and atlas */
    uint8_t view_agent[MG_MAX_AGENTS];
    uint8_t agent_color_idx[MG_MAX_AGENTS];
    int32_t any_spawn_delay;                                      /* 1 if some spawn_delay != 0 */
    int32_t spawn_delay[MG_MAX_AGENTS];                           /* agents.py:34; base.py:409-412, 503-506 */
    uint32_t prestige_mask;                                       /* bit k: agent k's colour is 'prestige' */
    uint8_t prestige_amax[4];                                     /* max sprite alpha per dir at tile_size */
    int32_t prestige_sprite_tile;                                 /* atlas tile index of the 4 un-bordered white
                                                                   * agent sprites (dir 0..3) appended to the atlas */
    double prestige_beta[MG_MAX_AGENTS], prestige_scale[MG_MAX_AGENTS];   /* agents.py:31-32, 141-153 */
    int32_t any_hide;                                             /* 1 if any mask below is non-zero */
    uint32_t hide_agent_mask;                                     /* bit k: agent k hides type 'Agent' */
    const uint32_t* hide_by_obj; /* device uint32 [n_obj] or NULL (nobody hides an object): bit k of entry o = agent k hides
                             * object id o (hide_item_types, base.py:441-449) */
    const MgObjDesc* obj;   /* device, [n_obj] */
    const uint8_t* atlas;   /* device, [4 orientations][n_tiles][tile_size*tile_size*3], pre-rotated.
                             * tile 0 = shadow; 1+o = object o alone (o=0: empty tile);
                             * 1+n_obj+(slot*n_agents+k)*4+d = slot's object with agent k facing d */
    const uint8_t* spawn_reject; /* device [cells_stride] or NULL: agent_spawn_kwargs['reject_fn'] (base.py:411, 505,
                             * 643 -> :700-701) tabulated over the grid, index x*H + y, != 0 = rejected: a rejected
                             * draw is a spent try, exactly like a cell that does not accept the agent */
} MgConfig;

typedef struct MgState {
    uint8_t* grid;
    uint64_t* agents;
    uint32_t* mt;
    int32_t* mt_pos;
    int32_t* step_count;
    uint8_t* done;
    int32_t* error;
    double* prestige;     /* [B][n_agents] agent.prestige (agents.py:141-153); NULL unless prestige_mask != 0 */
    uint32_t* mt_head;    /* [B][MG_MT_HEAD] */
    int32_t* error_flag;  /* [1] or NULL.  A kernel that records a per-env error in error[b] also ORs 1 into this word
                           * with a system-scope atomic, so the word may live in host-mapped memory
                           * (mg_host_flag_alloc) and be polled by the host without a stream synchronize: the
                           * reference raises inside step() (base.py:619-620); a batched host learns of an error
                           * without giving up its asynchronous launch queue.  Never cleared by the library. */
} MgState;

/* `_gen_grid` as data: a static template (walls / put_obj results) + ordered random placements */
typedef struct MgGenOp {
    int32_t obj, count, max_tries; /* max_tries >= 1: place_obj(obj, max_tries) x count (rejection sampling, below).
                                   * max_tries == 0 (ABI 4): a STATIC edit that `_gen_grid` makes after a random placement
                                   * (put_obj / grid.set / a wall helper, base.py:655-662, 160-176): `obj` (0 = None) is
                                   * written into every cell of [x0,x1) x [y0,y1), replacing what is there; no RNG draw.
                                   * Static edits BEFORE the first placement are part of template_grid.
                                   * max_tries < 0: a DRAW, `self._rand_int(x0, x1)` inside `_gen_grid`: draw[obj] = x0 +
                                   * bounded(x1 - x0 - 1) on the env's RNG (numpy's randint: masked rejection; a one-value
                                   * range consumes nothing), obj in [0, MG_GEN_DRAWS); count, y0, y1 and reject are unused.
                                   * The draws live for the duration of ONE reset; they are no part of MgState; every
                                   * register is 0 when a reset begins.
                                   * max_tries == MG_GEN_PARAM (-2; a value that was meaningless before: ABI 6 still): a PARAM,
                                   * `self._param(name, x0, x1)` inside `_gen_grid`: draw[obj] = clamp(params[env][y0], x0, x1 - 1)
                                   * — a register loaded from the env's row of the parameter table (MgGenProgram.template_grid)
                                   * instead of the RNG; no RNG word.  y0 in [0, MG_GEN_DRAWS) is the table column, [x0, x1) the
                                   * declared interval (within 0..255).  The clamp makes a table of any bytes safe: no value moves
                                   * a fill or a sampling rectangle outside what was proved for the interval.  Guardable like any
                                   * op.  max_tries == -1 is the RNG draw.
                                   * max_tries == MG_GEN_EDITS (-3; meaningless before: ABI 6 still): EDITS, the env's own list of
                                   * cell edits — `count` = K entries (1 .. MG_GEN_MAX_EDITS) of uint8_t edits[B][K][4] behind the
                                   * parameter table (MgGenProgram.template_grid), an entry being (x, y, obj, on).  For env b and
                                   * k = 0 .. K-1 in order: if on != 0, x < W, y < H and obj < n_obj, cell (x, y) becomes obj (0
                                   * empties it) — what a static edit (max_tries == 0) does to one cell; a later entry wins.  Any
                                   * other entry is ignored: no error, no write outside the env's grid slice, whatever bytes the
                                   * table holds.  No draw register, no RNG word; obj's low byte, the rectangle and reject are
                                   * unused (0, 0, -1); guardable like any op.
                                   * `count` of a placement may carry MG_GEN_SYM too (`const +- draw[r]`, illegal before): evaluated
                                   * per env like the rectangle's operands, below 0 counts as 0; that many consecutive place_obj
                                   * calls, consuming the same RNG words in the same order.
                                   * `obj` is the object id (the draw register of a DRAW) in its LOW BYTE.  With MG_GEN_GUARD
                                   * (bit 30) the op is GUARDED — a branch of `_gen_grid` on a draw, flattened: r = bits 24-26,
                                   * hi = bits 16-23, lo = bits 8-15, and the op runs only in an env with lo <= draw[r] <= hi.
                                   * A guard that is false skips the op entirely: no RNG word, no write, no error, and a guarded
                                   * DRAW leaves its register as it was.  Without the bit the upper bits are zero. */
    int32_t x0, y0, x1, y1;       /* sampling rectangle [x0,x1) x [y0,y1): place_obj(top=, size=) clamped
                                   * to the grid (base.py:692-695); the whole grid by default.  Each of the four is a plain
                                   * integer or, with MG_GEN_SYM, `const +- draw[r]` of an EARLIER draw op — evaluated per env
                                   * when the op runs (a draw's own x0 / x1 as well).  A place or fill rectangle with such an
                                   * operand is clamped to the grid on the device (for a place op that is the reference's
                                   * clamp); a place op whose clamped rectangle is empty records MG_ERR_VALUE (randint with
                                   * low >= high).  The values a draw can take must lie in 0..255. */
    int32_t reject;               /* place_obj(reject_fn=) (base.py:690, 700-701): the callback tabulated once over the
                                   * grid — row `reject` of MgGenProgram.reject, -1 = none.  A per-draw Python callback
                                   * cannot run on the device; a function of the position alone is a table. */
} MgGenOp;
typedef struct MgGenProgram {
    const uint8_t* template_grid; /* device, [cells_stride].  A program that holds a PARAM op (MG_GEN_PARAM) is followed DIRECTLY by
                                   * the parameter table: uint8_t params[B][MG_GEN_DRAWS] at template_grid + cells_stride, row = env,
                                   * column = the op's y0; read at every reset of an env (a change takes effect at the env's next
                                   * reset).  A program that holds an EDITS op (MG_GEN_EDITS) has, whether it holds a PARAM op or not,
                                   * that table's B * MG_GEN_DRAWS bytes and DIRECTLY behind them uint8_t edits[B][K][4] (K = the op's
                                   * count) at template_grid + cells_stride + B * MG_GEN_DRAWS: rows of 4-byte aligned entries
                                   * (x, y, obj, on), read at every reset of an env like the parameters.
                                   * Every other program is the bytes it was and needs no tail.  (Not behind `ops`: the fused
                                   * kernel reads programs of at most 32 ops from an LDS copy; template_grid is read in place.) */
    int32_t n_ops;
    const MgGenOp* ops;           /* DEVICE, [n_ops]: placements and late static edits, in `_gen_grid` order — upstream's `_gen_grid`
                                   * is free Python of any length (marlgrid/envs); the program lives in device memory, not in the
                                   * launch arguments.  The library cannot look into it from the host: the caller hands over ops
                                   * with 0 <= obj < n_obj (>= 1 for placements), count >= 0 and reject in [-1, n_reject); a rectangle
                                   * of plain integers is non-empty and inside the grid (one with a draw operand is clamped) */
    const uint8_t* reject;        /* device, [n_reject][cells_stride], index x*H + y, != 0 = rejected; NULL if no op
                                   * has a reject table */
    int32_t n_reject;
} MgGenProgram;

int32_t mg_abi_version(void);
/* sizeof of the structs of this header as THIS build sees them: out[0..6] = MgConfig, MgState, MgObjDesc, MgGenOp,
 * MgGenProgram, MgPlaceTuning, MgPlaceStats.  A binding compares them with its own mirror of the structs at load time
 * (the layouts have no other self-description; MG_ABI_VERSION changes whenever one of them does).  Returns 7. */
int32_t mg_struct_sizes(int32_t out[7]);
/* "<library> gfx950 abi<N> <source id>": which build answered (bench.py echoes it) */
const char* mg_build_info(void);
const char* mg_error_string(int32_t code);

/* keys: device uint32 [B][MG_KEY_WORDS] (sha512-derived words, host computed), key_len: device
 * int32 [B] (1 or 2).  Writes mt [B][624], mt_head [B][16] (the stream's first 16 outputs) and
 * mt_pos [B] (= 16: the next word to regenerate). */
int32_t mg_mt_seed(int32_t B, const uint32_t* keys, const int32_t* key_len, uint32_t* mt,
                   int32_t* mt_pos, uint32_t* mt_head, void* stream);

/* env_mask: device uint8 [B] or NULL (= all); only envs with mask != 0 are reset. */
int32_t mg_reset(const MgConfig* cfg, const MgState* st, const MgGenProgram* prog,
                 const uint8_t* env_mask, void* stream);

/* Replayable levels: a level is a seed, and playing it is `env.seed(s); env.reset()` (base.py:371-374) — the episode that
 * follows a generator freshly seeded with s.  A bank holds such generators: bank_mt uint32 [L][624], bank_pos int32 [L],
 * bank_head uint32 [L][16] (what mg_mt_seed writes per env), bank_seed int64 [L] with -1 = empty slot; bank_mt and bank_head
 * 16-byte aligned.  All device memory, caller-owned.
 *
 * mg_level_seed: row i of n puts seeds[i] (device int64) into slot slots[i] (device int64 [n]; NULL: slot i), hashing the
 * seed on the device as gym's seeding.np_random does.  row_mask: device uint8 [n] or NULL (= all), rows with mask != 0 only.
 * A seed < 0 empties the slot (bank_seed = -1, generator untouched); a slot outside [0, n_slots) is skipped; two rows of one
 * call naming one slot are the caller's error. */
int32_t mg_level_seed(int32_t n, const int64_t* seeds, const int64_t* slots, const uint8_t* row_mask, int32_t n_slots,
                      uint32_t* bank_mt, int32_t* bank_pos, uint32_t* bank_head, int64_t* bank_seed, void* stream);
/* mg_level_apply (base.py:371-374), in front of the launch that resets: every *selected* env b whose level_of_env[b] (device
 * int64 [B]) names a filled slot gets that slot's generator in place of its own (st->mt, mt_pos, mt_head), its agents'
 * headings set to 0 (a reset keeps them: the level starts as in an env made for it) and episode_level[b] = bank_seed[slot]; a selected env whose level is < 0, >= n_slots or empty keeps its running stream and
 * gets episode_level[b] = -1 (free-running).  Selected by `rule`: MG_LEVEL_PENDING — the envs whose episode has ended, read
 * off the state as the next-step reset of mg_*_ep reads it (never st->done) —, MG_LEVEL_MASK — env_mask as mg_reset takes
 * it —, MG_LEVEL_PUBLISH — none.  Last, out_level[b] = episode_level[b] for every env (out_level: device int64 [B] or NULL).
 * Only B, n_agents and max_steps of cfg are read. */
#define MG_LEVEL_PUBLISH 0
#define MG_LEVEL_PENDING 1
#define MG_LEVEL_MASK 2
int32_t mg_level_apply(const MgConfig* cfg, const MgState* st, int32_t rule, const uint8_t* env_mask,
                       const int64_t* level_of_env, int32_t n_slots, const uint32_t* bank_mt, const int32_t* bank_pos,
                       const uint32_t* bank_head, const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level,
                       void* stream);
/* mg_level_apply_rows: mg_level_apply for a bank whose levels also carry a parameter row and an edit list.  Everything above,
 * and for every selected env that takes a slot (>= 0, filled) the slot's rows are copied over the env's, in the same launch, by
 * the wave that copies the generator: bank_params uint8 [L][MG_GEN_DRAWS] -> env_params uint8 [B][MG_GEN_DRAWS] and bank_edits
 * uint8 [L][K][4] -> env_edits uint8 [B][K][4] — the env's tables are the ones behind its reset programs' template
 * (MgGenProgram.template_grid), so the reset in the launch that follows reads the level's rows, and the env's rows afterwards
 * show what the running episode was built from.  Free-running and unselected envs keep their rows.  A pair (bank_*, env_*) is
 * given whole or NULL — NULL: that part is not copied —; 1 <= K <= MG_GEN_MAX_EDITS with an edit pair, else 0; the four
 * pointers 4-byte aligned.  All device memory, caller-owned. */
int32_t mg_level_apply_rows(const MgConfig* cfg, const MgState* st, int32_t rule, const uint8_t* env_mask,
                            const int64_t* level_of_env, int32_t n_slots, const uint32_t* bank_mt, const int32_t* bank_pos,
                            const uint32_t* bank_head, const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level,
                            const uint8_t* bank_params, const uint8_t* bank_edits, int32_t K, uint8_t* env_params,
                            uint8_t* env_edits, void* stream);

/* Goal distance (no reference counterpart: a static analysis of the level a learner cannot get from a rollout).  For every
 * selected env — env_mask: device uint8 [B] or NULL (= all), as mg_reset takes it — and the env's grid as it is now:
 * agent_dist[b][k] (device int32 [B][n_agents]) = the smallest number of actions `left`, `right`, `forward` (base.py:530-585)
 * after which agent k's `forward` ENTERS a goal cell, other agents ignored, nothing toggled, picked up or dropped; -1: no such
 * sequence, or the agent is in no cell (not active — not yet spawned, done —, or MG_AF_EVICTED).  field (device int32
 * [B][W][H][4] or NULL): the same number for every state, field[b][x][y][dir]; -1 where there is none and on cells an agent
 * cannot stand on.  Rows of unselected envs are not written.
 *   goal cell: an object with reward_kind == 1 and MG_OF_ENDS_EPISODE.  Free cell: id 0, or MG_OF_CAN_OVERLAP without
 *   MG_OF_ENDS_EPISODE (floor, bonus tiles, open doors).  Everything else blocks — walls, keys, balls, boxes, closed and locked
 *   doors, lava —, and so does the outside of the grid: nothing wraps, a missing border wall included.  Entering a goal ends the
 *   agent's episode, so goal cells are never passed through; an agent that STANDS on a goal has not entered it, may turn there
 *   and leave, and must enter a goal cell from outside.
 * One launch, one wave per selected env, a reverse breadth-first search by levels over bit planes: in registers where
 * 4 W <= 64 and H <= 64, in LDS otherwise (14 * 8 * W * ceil(H / 64) + 128 bytes per env: 111.7 KiB at 255 x 255); at most
 * 4 W H + 1 levels; without `field` an env stops once its agents are all labelled.  With ghost_mode off other agents can block
 * a path: the number is then a lower bound.
 * Only B, W, H, n_agents, cells_stride, n_obj and obj of cfg are read (1 <= W, H <= 255), and grid and agents of st.
 * MG_E_ARG: a NULL cfg, st, agent_dist, grid, agents or obj, or a size outside those bounds; MG_E_UNSUPPORTED: the planes do
 * not fit LDS (no W, H <= 255 gets there). */
int32_t mg_goal_distance(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, int32_t* agent_dist, int32_t* field,
                         void* stream);
/* ... with the kernel named: path 0 as above, 1 the register-resident kernel (MG_E_UNSUPPORTED unless 4 W <= 64 and H <= 64),
 * 2 the LDS kernel; MG_E_ARG for any other path.  NOT for hosts: it exists so that the project's own tests and measurements can
 * hold the two kernels to each other, it may change or go with either kernel, and no binding outside this repository should
 * depend on it — mg_goal_distance is the call. */
int32_t mg_goal_distance_path(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, int32_t* agent_dist,
                              int32_t* field, int32_t path, void* stream);

/* Solve distance (no reference counterpart): mg_goal_distance's question with keys and doors in play.  For every selected env —
 * env_mask as above — and every agent k of it: agent_dist[b][k] (device int32 [B][n_agents]) = the smallest number of actions
 * out of `left` (0), `right` (1), `forward` (2), `pickup` (3) and `toggle` (5) after which agent k's `forward` ENTERS a goal
 * cell — on the env's grid as it is now, the agent carrying what it carries now (MG_AG_CARRY), other agents ignored, under the
 * step's own rules (base.py:530-613); -1: no such sequence, or the agent is in no cell, or it stands on a cell that is neither
 * free nor a goal (a door shut on it included).  `drop` and `done` are never used, so an agent picks up at most ONE object:
 * two locked doors of two colours in a row have no path.
 *   Cells are mg_goal_distance's free / goal / blocked; nothing wraps, lava blocks, goals are entered and never crossed.  A
 *   blocked cell becomes free in two ways.  An ITEM — a blocked cell whose object has MG_OF_CAN_PICKUP — is taken by `pickup`
 *   with empty hands.  A SHUT DOOR — MG_OF_IS_DOOR without MG_OF_CAN_OVERLAP and MG_OF_IS_BOX — is opened by `toggle`: one
 *   action if it is not locked (-> toggle_next), two if it is (-> unlock_next, a closed door, -> that door's toggle_next), the
 *   second only for an agent that holds an MG_OF_IS_KEY object of the door's color_idx.  A door counts as openable only if the
 *   id it ends as is a free cell; doors are never closed again; a box is never toggled.
 *   Of each env the first max_doors (0 .. 4) shut doors and the first max_items (0 .. 3) items in grid index order x * H + y are
 *   TRACKED; those beyond the caps block and are never touched.  env_exact[b] (device uint8 [B] or NULL) = 1 iff the env has
 *   no more of either than the caps; where it is 0 every value is -1 or NOT SMALLER than the uncapped one.  For an agent that
 *   already carries something no item is tracked (it cannot pick up).
 * agent_action[b][k] (device int8 [B][n_agents] or NULL): the first action of such a path — the lowest action id whose
 * successor state lies one action nearer (two for the first toggle of a locked door) —, 6 (`done`) where there is no path.
 * After that action is stepped, the call on the new state gives exactly one less.  Rows of unselected envs are not written.
 * One launch, one wave per selected env: mg_goal_distance's reverse search by levels over bit planes, in LDS, over the up to
 * 2^D (1 + K) LAYERS (set of tracked doors opened, tracked item picked up or none) of the env's own D <= max_doors doors and
 * K <= max_items items at once, the few edges between layers (pickup, open: cost 1; unlock and open: cost 2) taken per level
 * from the states that face the object; once per class of carry among the env's agents.  LDS per env:
 * 8 W ceil(H / 64) (2 + 12 (1 + max_items) 2^max_doors) + 1024 bytes (mg_solve_distance_lds_bytes) — 18.1 KiB at 15 x 15 with
 * (2, 2); 255 x 255 fits with (0, 0) only.
 * Only B, W, H, n_agents, cells_stride, n_obj and obj of cfg are read (1 <= W, H <= 255), and grid and agents of st.
 * MG_E_ARG: a NULL cfg, st, agent_dist, grid, agents or obj, a size outside those bounds, max_doors outside 0 .. 4 or max_items
 * outside 0 .. 3; MG_E_UNSUPPORTED: the layers need more than 160 KiB of LDS — worked out on the host: nothing is launched,
 * nothing written. */
int32_t mg_solve_distance(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, int32_t max_doors, int32_t max_items,
                          int32_t* agent_dist, int8_t* agent_action, uint8_t* env_exact, void* stream);
/* the LDS bytes per env mg_solve_distance needs for the shape and the caps (it runs iff they are <= 160 KiB); MG_E_ARG as above */
int32_t mg_solve_distance_lds_bytes(int32_t W, int32_t H, int32_t max_doors, int32_t max_items);

/* Lookahead (no reference counterpart): "what happens if these agents do THIS for the next T steps", asked of the simulator
 * without doing it.  A second, SHADOW MgState — caller-owned, R rows, its error_flag NULL — is filled with copies of env rows
 * (mg_fork_rows) and stepped through one plan of T actions per row in one launch (mg_rollout); the env's state is only read.
 *
 * mg_fork_rows: for r in [0, R), row d = dst_of_row[r] (device int64 [R]; NULL: d = r) of `dst` becomes a copy of row
 * s = src_of_dst[r % m] (device int64 [m]; NULL: s = r % m) of `src`: grid slice, agent records, generator (mt, mt_pos, mt_head),
 * step_count, done, error, and prestige when cfg->prestige_mask != 0.  cfg->B is the number of rows of `src`; only B, n_agents,
 * cells_stride and prestige_mask of cfg are read.  s outside [0, cfg->B): the row is made INERT — an ended episode (every
 * record MG_AF_DONE, step_count INT32_MAX, done 1, error 0, grid and generator zero) that mg_rollout never steps.  d outside
 * [0, dst_B): nothing is written for r.  Two r naming one d are the caller's error; `src` and `dst` must not overlap.
 * One wave per row, 16-byte vectors for the 2 496-byte generator, its head and the grid slice (bytes where a slice is not
 * 16-byte aligned); the R / m rows that read one source row are neighbours in the launch.  m >= 1 and R a multiple of m.
 * MG_E_ARG: a NULL cfg or state array, mt / mt_head of either state not 16-byte aligned, R, m or dst_B out of range. */
int32_t mg_fork_rows(const MgConfig* cfg, const MgState* src, const MgState* dst, const int64_t* src_of_dst,
                     const int64_t* dst_of_row, int32_t dst_B, int32_t R, int32_t m, void* stream);
/* mg_rollout: every row r of the shadow state `st` (cfg->B = R rows, plan-major: r = p * m + j — plan p of env j —, K = R / m
 * plans) is stepped T times as mg_step with auto_reset == NULL would step it, step t with actions[p][t][j][.]:
 *   actions  device [K][T][m][n_agents], element size `action_bytes` in {1, 4, 8}
 *   rewards  device float32 [K][T][m][n_agents];  done: device uint8 [K][T][m]
 *   errors   device int32 [R] or NULL: the first MG_ERR_* a step of the row recorded in this call, 0 for none (st->error[r] is
 *            cleared when the call begins: what the copied env had recorded is the env's)
 * with one difference: a rollout STOPS AT ITS EPISODE'S END.  "Ended" is read off the row's state before each step — step_count >=
 * max_steps, or every record MG_AF_DONE: what next-step reset reads, never st->done —; from then on the row is frozen, its
 * rewards are 0 and done is 1.  A row whose episode had ended when it was copied, and an inert row, are frozen from t = 0.
 * Nothing resets, no reset program is read, st->error_flag should be NULL.  One launch, one lane per row, the bodies mg_step
 * runs (so the rewards are bit-identical to T mg_step calls); results are independent of K and of the other rows.
 * MG_E_ARG: what mg_step answers it for, a NULL done, T < 0, m < 1, or cfg->B no multiple of m. */
int32_t mg_rollout(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, int32_t T, int32_t m,
                   float* rewards, uint8_t* done, int32_t* errors, void* stream);

/* Exploration maps (no reference counterpart).  Per env b and agent k, caller-owned device memory, kept up to date by ONE call
 * after every mg_reset (with the reset's mask) and after every step launch (mask NULL), i.e. once per observation returned:
 *   seen         uint8 [B][n_agents][W][H], index [b][k][x][y]: 1 iff cell (x, y) was inside agent k's view AND VISIBLE in at
 *                least one observation since the env's running episode began
 *   visits       int32 [B][n_agents][W][H]: the number of those observations in which agent k was placed (MG_AF_PLACED) on (x, y)
 *   new_cells    int32 [B][n_agents]: how many cells this call added to seen[b][k]
 *   visit_count  int32 [B][n_agents]: visits[b][k] at agent k's own cell after this call's increment; 0 for an agent in no cell
 * VISIBLE is exactly the vis_mask of the reference's gen_obs_grid(agent) (base.py:418-451): crop at get_view_exts, rotate dir + 1
 * times, process_vis — all ones with see_through_walls, all zeros for a viewer that is not MG_AF_ACTIVE (base.py:420-425),
 * clipped to the grid, the transparency that of the grid's own object (base.py:103-106); hide_item_types plays no part.  It is
 * taken on the state `st` holds, which is the state the returned observation shows.
 * A FRESH EPISODE CLEARS FIRST: an env whose step_count is 0 has just begun an episode — mg_reset, the same-step reset inside a
 * step, or the next-step reset call; every other step leaves step_count >= 1 — and seen[b], visits[b] of the launch's agents are
 * zeroed before the observation is accumulated.  So with a same-step reset the values after a finishing step are those of the
 * new episode's first observation; with next-step reset the terminal step still accumulates and the reset call clears.
 * cfg is a view group's config: the launch writes the rows of cfg->view_agent[0 .. n_view) (every agent when n_view == 0) of the
 * envs with env_mask[b] != 0 (NULL: every env); rows of other agents and of unselected envs are not touched.  One launch, no
 * atomics, nothing the host has to read; every size mg_encode_views takes (grids to 255 x 255, views to MG_MAX_VIEW).
 * MG_E_ARG: what mg_encode_views answers it for, or a NULL array. */
int32_t mg_explore_update(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, uint8_t* seen, int32_t* visits,
                          int32_t* new_cells, int32_t* visit_count, void* stream);

/* Memory maps (no reference counterpart): mg_explore_update, and with it each agent's LAST VIEW OF EVERY CELL.  A caller that
 * keeps them calls this INSTEAD OF mg_explore_update, at the same places (after every mg_reset with its mask, after every step
 * launch with NULL): one launch, the view chain run once.  seen, visits, new_cells, visit_count: exactly as mg_explore_update
 * leaves them.  Two more caller-owned device arrays:
 *   memory     uint8 [B][n_agents][W][H][4], 4-byte aligned, index [b][k][x][y] = (type, colour, state, known): the first three
 *              bytes are the triple cell (x, y) had in the most recent observation of agent k in which the cell was inside its
 *              view AND VISIBLE — byte for byte what mg_encode_views writes at the view cell that maps to (x, y) on the same
 *              state: the shadow cast applied, hide_item_types applied (a hidden object shows the agent on it or (0, 0, 0)), an
 *              agent standing there encoded as (agent type, its colour, its heading); known = 1 once the cell has been seen this
 *              episode, so a seen empty cell (0, 0, 0, 1) differs from a cell never seen (0, 0, 0, 0)
 *   seen_step  int32 [B][n_agents][W][H]: st->step_count[b] at that most recent observation; -1 where the cell was never seen
 * The rules are mg_explore_update's: an env whose step_count is 0 is cleared first (memory to 0, seen_step to -1); an inactive
 * viewer sees nothing and changes nothing, what it remembered stays; the launch writes the rows of cfg's viewers in the selected
 * envs only.  After every call memory[..][3] == seen, (seen_step >= 0) == seen, and every cell visible in the observation has
 * seen_step == step_count[b].  No atomics (a view map is injective, two pairs never share a plane), nothing read back.
 * MG_E_ARG: what mg_explore_update answers it for, a NULL array, or a `memory` that is not 4-byte aligned. */
int32_t mg_memory_update(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, uint8_t* seen, int32_t* visits,
                         int32_t* new_cells, int32_t* visit_count, uint8_t* memory, int32_t* seen_step, void* stream);

/* actions: device [B][n_agents], element size `action_bytes` in {1,4,8} (little-endian ints).
 * rewards: device float32 [B][n_agents].  Sets st->done[b].
 * auto_reset: NULL, or the reset program: an env whose episode ends in this step (done[b] = 1) starts
 * its next episode inside the same launch, exactly as mg_reset masked by the done flags would
 * (done[b] keeps reporting the end; step_count[b] = 0 afterwards). */
int32_t mg_step(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                float* rewards, const MgGenProgram* auto_reset, void* stream);

/* MultiGridEnv.step as ONE launch: mg_step (arguments as above) and mg_render_obs fused — the wave that
 * renders an env steps it first (one lane per env), so the whole base.py:501-653 step is a single kernel and
 * nothing separates the action loop from the observation raster.  Results are identical to mg_step
 * followed by mg_render_obs. */
int32_t mg_step_render(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                       float* rewards, const MgGenProgram* auto_reset, uint8_t* obs, void* stream);

/* mg_step_render that also writes MultiGrid.encode (base.py:196-214) of the stepped batch — what mg_encode(cfg, st,
 * NULL, encode_out) would write right after it — from the same launch: the wave that has stepped and drawn its envs
 * still holds their grids and records.  encode_out: device uint8 [B][W][H][3] (any alignment).  +2.4 % bytes on
 * MarlGrid-3AgentCluttered15x15-v0 instead of a second launch.  Compiled into instantiations of the step kernel of their
 * own: view sizes 7, 9 and those above 9 with 8-pixel tiles, view 7 with 5-pixel tiles.  MG_E_UNSUPPORTED —
 * nothing launched, call mg_step_render and mg_encode — for every other shape, and when n_obj + 4 n_agents > 256 (object
 * ids and agent marks do not share a byte), with 'prestige' agents, or when the grid or the atlas does not fit LDS. */
int32_t mg_step_render_encode(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                              float* rewards, const MgGenProgram* auto_reset, uint8_t* obs, uint8_t* encode_out,
                              void* stream);

/* mg_step_render into a buffer that still holds what an earlier call of this function wrote there: the bands — one tile row of
 * one agent's image, tile_size pixel rows — whose tiles are the ones that buffer was drawn from are not stored again.
 * signature: device memory the caller keeps WITH `obs`, one per observation buffer, 16-byte aligned,
 * B * MG_DELTA_SIG_BYTES(n_agents, view_size) bytes; per env the tile (orientation and overlay included) of every view cell of
 * what `obs` holds: read, compared exactly — no hashes —, and rewritten by the call.  Its contents mean nothing to the caller.
 * flags: MG_DELTA_FORCE — every band counts as changed and the signature is only recorded: the first call for a pair
 * (obs, signature), and every call after anything else wrote into `obs` (mg_render_obs, the caller itself) or the atlas or the
 * object table behind cfg changed — or, in stream order and therefore also for launches replayed from a captured graph, a
 * signature filled with 0xFF bytes (a 0xFF fill is no tile in either layout the library keeps there — 16-bit entries, or one-byte
 * codes where the configuration's tiles fit a byte —: every band compares unequal).  The bytes in `obs` after the
 * call are mg_step_render's.
 * MG_E_UNSUPPORTED — nothing launched, call mg_step_render — unless: view 7 with 8-pixel tiles, at most 3 agents, no 'prestige'
 * agent, grid and atlas in LDS. */
#define MG_DELTA_FORCE 1u
#define MG_DELTA_SIG_BYTES(n_agents, view_size) ((((n_agents) * (view_size) * (view_size) * 2) + 15) / 16 * 16)
int32_t mg_step_render_delta(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                             float* rewards, const MgGenProgram* auto_reset, uint8_t* obs, uint16_t* signature,
                             uint32_t flags, void* stream);

/* obs: device uint8 [B][n][P][P][3].  Optional debug outputs (NULL to skip):
 * view_cells uint8 [B][n][vs][vs] (object id of the rotated sub-grid, index [i][j]),
 * view_agent uint8 [B][n][vs][vs] (shown agent index or 0xFF), vis_mask uint8 [B][n][vs][vs]. */
int32_t mg_render_obs(const MgConfig* cfg, const MgState* st, uint8_t* obs, uint8_t* view_cells,
                      uint8_t* view_agent, uint8_t* vis_mask, void* stream);

/* MultiGridEnv.step like mg_step_render, but instead of pixels it writes every agent's
 * gen_obs_grid(agent) -> grid.encode(vis_mask) (base.py:418-451, 196-214) of the stepped state (mg_step, then
 * mg_encode_views, on `stream`).  views: device uint8 [B][n][vs][vs][3], index [i][j] as encode returns it, any alignment.
 * Per view cell the (type, colour, state) triple of what `grid.get` returns after hide_item_types — an agent standing on an
 * object is not encoded, the bottom agent of a stack on an empty cell is —; invisible cells, empty cells, cells outside the
 * grid and every cell of an inactive agent's view are (0, 0, 0).  n_view must be 0 (view groups: mg_step, then
 * mg_encode_views per group). */
int32_t mg_step_encode_views(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                             float* rewards, const MgGenProgram* auto_reset, uint8_t* views, void* stream);
/* ---- episode boundaries under auto-reset ---------------------------------------------------------------------------
 *
 * What a learner needs at the end of an episode and cannot get from outside the launch once the reset is fused into
 * the step: the observation of the terminal state, WHY the episode ended, and its return and length.  MgEpisode is the
 * extra argument of the mg_*_ep entry points below (each its twin plus `ep`; ep == NULL: exactly the twin).  All pointers
 * are caller-owned device memory; NULL = that output is not wanted.  Not part of mg_struct_sizes: mg_episode_struct_size.
 *
 * reset_mode 0, SAME-STEP: the twin's behaviour — with a reset program an env whose episode ends is reset inside the
 * launch; the outputs below are written BEFORE that reset (which also zeroes the env's accumulators).
 * reset_mode 1, NEXT-STEP (needs the reset program): the step that ends an episode does NOT reset — done[b] = 1 and the
 * state (and whatever the launch renders or encodes from it) is the terminal one.  The env's NEXT step call is its reset:
 * "ended" is read off the persistent state — step_count[b] >= max_steps (base.py:649), or every agent record carries
 * MG_AF_DONE (base.py:627-649; with `respawn` none keeps it) —, the env's action row is ignored altogether (no
 * MG_ERR_VALUE for an unknown action), nothing spawns late, nothing is shuffled (no RNG draw), every reward is 0, and the
 * env is reset exactly as mg_reset would (same draws): step_count[b] = 0, done[b] = 0, accumulators 0, out_return 0,
 * out_length 0, out_flags MG_EPF_RESET.
 * mg_reset knows nothing of the accumulators: a caller that resets envs by hand zeroes their ep_return rows. */
#define MG_EPF_TERMINATED 1 /* done, and every agent is done (the `all(agent.done)` half of base.py:649) */
#define MG_EPF_TRUNCATED 2  /* done and not terminated: step_count >= max_steps alone (base.py:649) */
#define MG_EPF_RESET 4      /* this call was the env's reset (next-step mode) */
typedef struct MgEpisode {
    int32_t reset_mode;     /* 0 same-step, 1 next-step */
    int32_t reserved0;
    double* ep_return;      /* [B][n_agents] persistent: the running episode's sum of the step rewards (the float32 values the
                             * step writes — base.py:576-581 —, added in float64, one add per step) */
    double* out_return;     /* [B][n_agents] per step: that sum including this step's reward, before any reset — where done[b],
                             * the finished episode's return.  Needs ep_return. */
    int32_t* out_length;    /* [B] per step: step_count (base.py:512) after this step, before any reset */
    uint8_t* out_flags;     /* [B] per step: MG_EPF_* */
} MgEpisode;
int32_t mg_episode_struct_size(void);   /* sizeof(MgEpisode) as this build sees it */
/* MG_E_ARG (no device access): reset_mode outside {0, 1}; reset_mode 1 without a reset program; out_return without ep_return. */
int32_t mg_step_ep(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                   const MgGenProgram* auto_reset, const MgEpisode* ep, void* stream);
/* mg_step_render with `ep`.  Compiled into instantiations of the step kernel of their own (the plain ones run at their
 * register limit), for the shapes mg_step_render_encode has: views 7, 9 and those above 9 with 8-pixel tiles, view 7 with
 * 5-pixel tiles.  MG_E_UNSUPPORTED — nothing launched, call mg_step_ep and mg_render_obs — for every other shape, with
 * 'prestige' agents, or when the grid or the atlas does not fit LDS.  There is no _ep twin of mg_step_render_encode:
 * mg_step_render_ep, then mg_encode. */
int32_t mg_step_render_ep(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                          const MgGenProgram* auto_reset, uint8_t* obs, const MgEpisode* ep, void* stream);
int32_t mg_step_encode_views_ep(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                                float* rewards, const MgGenProgram* auto_reset, uint8_t* views, const MgEpisode* ep,
                                void* stream);
/* mg_step_render_delta that also writes what mg_step_render_encode (encode_out), mg_step_render_ep (ep) or BOTH would — the one
 * launch with the encode and the episode outputs together; it has no non-delta twin.  obs, signature, flags: as for
 * mg_step_render_delta (the same signature serves both calls: a buffer may be written by either); encode_out, ep: as for the
 * two calls named, either may be NULL.  The bytes in `obs`, in `encode_out` and in the episode outputs after the call are
 * those of mg_step_render_ep (mg_step_render without ep) followed by mg_encode.
 * MG_E_ARG (no device access): encode_out and ep both NULL (that call is mg_step_render_delta), a NULL or misaligned signature,
 * an unknown flag, an MgEpisode mg_step_ep would refuse.
 * MG_E_UNSUPPORTED — nothing launched, call mg_step_render_ep / mg_step_render_encode / mg_encode — unless mg_step_render_delta
 * has the shape (view 7 with 8-pixel tiles, at most 3 agents, no 'prestige' agent, grid and atlas in LDS) and, with encode_out,
 * mg_step_render_encode has it too (n_obj + 4 n_agents <= 256, the table fits LDS beside four waves). */
int32_t mg_step_render_delta_ex(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                                float* rewards, const MgGenProgram* auto_reset, uint8_t* obs, uint16_t* signature,
                                uint32_t flags, uint8_t* encode_out, const MgEpisode* ep, void* stream);

/* ---- the observation kernel specialised on demand (mg_rtc.hip) -------------------------------------------------------
 *
 * The library ships ~100 instantiations of its observation kernel; a (view_size, tile_size) pair off that table runs the
 * instantiation that reads both at run time (mg_render_kernel_name's bits), 2-2.4x slower.  mg_render_specialize compiles
 * the instantiation the configuration would have if it were on the table — from the library's own headers, the files next
 * to it (marlgrid_amd/csrc/ and include/ of the tree it was built in; refused when they are not the ones it was built from),
 * with hipRTC (libhiprtc is loaded at the first call; the library loads without it) — and returns a
 * handle that mg_step_render_spec / mg_render_obs_spec launch instead of the table's entry.  Same arguments, same bytes
 * written as mg_step_render[_encode | _ep] / mg_render_obs.
 *
 * want: 0 the plain step / raster, 1 with the encode (mg_step_render_encode), 2 with the episode outputs (mg_step_render_ep).
 * arch: "gfx950", or NULL: the current device's.  cache_dir: a directory for compiled code objects (created if missing;
 * files are written under a temporary name and renamed, validated by length and checksum before they are loaded), or NULL.
 * flags: MG_SPEC_COMPILE_ONLY — compile (or read the cache) and fill `info` without touching a device; needs `arch`;
 * *handle stays NULL.  A handle belongs to the device that was current when it was made and to the shape (B's side of
 * 4096, agents, grid, view, tiles, tables) of `cfg`: the launch calls answer MG_E_ARG for a config whose pick differs.
 * Compiled code is kept per process: a second handle for the same instantiation and arch (another device, another env)
 * loads it without compiling (info->cache_hit = 1: memory, 2: cache_dir).
 *
 * MG_E_UNSUPPORTED, with the reason in info->reason: the table's instantiation is already the specialised one, or the
 * configuration is one that is not specialised ('prestige' agents, a grid or an atlas read in place, views under 3);
 * libhiprtc or the headers are missing; the compile failed; the instantiation needs scratch memory (spilled registers) even with 4-wave
 * workgroups — workgroups are stepped down 16 -> 8 -> 4 before that. */
#define MG_SPEC_COMPILE_ONLY 1u
typedef struct MgSpecInfo {
    char kernel_name[96];   /* "mg::render_kernel<VS, TS, WPB, V, RM>", mg_render_kernel_name's format */
    int32_t vs, ts, wpb, v, rm;
    int32_t lds_bytes;      /* LDS of one workgroup */
    int32_t lds_static;     /* 1: compiled in as a static array (workgroups over 64 KiB), 0: asked for at the launch */
    int32_t scratch_bytes;  /* private segment per work-item: 0 for every instantiation that is accepted */
    int32_t code_bytes;     /* the code object */
    int32_t cache_hit;      /* 0 compiled now, 1 taken from this process's memory, 2 read from cache_dir */
    int32_t table_is_ideal; /* MG_E_UNSUPPORTED because the table's instantiation is already the specialised one: nothing is missing */
    int32_t reserved0;
    double compile_seconds; /* 0 on a hit */
    char reason[256];       /* MG_E_UNSUPPORTED: why */
} MgSpecInfo;
int32_t mg_spec_info_struct_size(void);   /* sizeof(MgSpecInfo) as this build sees it */
int32_t mg_render_specialize(const MgConfig* cfg, int32_t want, uint32_t flags, const char* arch, const char* cache_dir,
                             void** handle, MgSpecInfo* info);
/* mg_step_render (encode_out == NULL, ep == NULL), mg_step_render_encode (encode_out) or mg_step_render_ep (ep) — the one
 * the handle was made for (MG_E_ARG otherwise) — through the handle's instantiation. */
int32_t mg_step_render_spec(void* handle, const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                            float* rewards, const MgGenProgram* auto_reset, uint8_t* obs, uint8_t* encode_out,
                            const MgEpisode* ep, void* stream);
/* mg_render_obs without the debug outputs (a handle made with want 0) */
int32_t mg_render_obs_spec(void* handle, const MgConfig* cfg, const MgState* st, uint8_t* obs, void* stream);
int32_t mg_render_spec_release(void* handle);   /* unloads the handle's module (on its device); NULL: nothing */
/* the sources mg_render_specialize compiles from, as the library read and accepted them: the count (0: missing, or not the
 * build's), and entry `i`'s name / text / length (tests: with the library's other sources they hash to mg_build_info's id) */
int32_t mg_rtc_source(int32_t i, const char** name, const char** text, int32_t* length);

/* The same views of the current state (after mg_reset / mg_step), for one view group's cfg: views [B][nv][vs][vs][3] with
 * nv = n_view, or n_agents when n_view == 0.  Tile size and atlas play no part. */
int32_t mg_encode_views(const MgConfig* cfg, const MgState* st, uint8_t* views, void* stream);

/* out: device uint8 [B][W][H][3]; vis_mask: device uint8 [B][W][H] or NULL. */
int32_t mg_encode(const MgConfig* cfg, const MgState* st, const uint8_t* vis_mask, uint8_t* out,
                  void* stream);

/* env_mask as in mg_reset. Replaces whatever is in the cell (base.py:655-662) — agents standing there included: they
 * leave the grid (MG_AF_EVICTED). */
int32_t mg_put_obj(const MgConfig* cfg, const MgState* st, int32_t obj, int32_t x, int32_t y,
                   const uint8_t* env_mask, void* stream);

/* Live placement (outside the reset program).  what >= 1: object id; what < 0: agent -(what+1), which
 * is lifted off the grid first and re-seated with the highest arrival rank (as a respawn does).
 * fixed_pos == NULL: rejection sampling in [x0,x1) x [y0,y1) with at most max_tries draws per env on the
 * env's RNG (place_obj, RecursionError recorded on failure); fixed_pos: device int32 [B][2], one attempt
 * at that cell (try_place_obj).  out_pos: device int32 [B][2] or NULL; out_ok: device uint8 [B] or NULL. */
int32_t mg_place(const MgConfig* cfg, const MgState* st, int32_t what, int32_t x0, int32_t y0, int32_t x1,
                 int32_t y1, int32_t max_tries, const int32_t* fixed_pos, const uint8_t* env_mask,
                 const uint8_t* reject, int32_t* out_pos, uint8_t* out_ok, void* stream);
/* reject: device uint8 [cells_stride] or NULL — place_obj(reject_fn=) tabulated (see MgGenOp.reject). */

/* Whole-grid human view of selected envs (caller-side format, not on the step path).
 * env_ids: device int32 [n_envs]; frame_atlas: device uint8 [n_tiles][ts][ts][3] (orientation 0,
 * same tile numbering as MgConfig.atlas) rendered at frame_tile_size (a multiple of 4, normally
 * TILE_PIXELS = 32); out: device uint8 [n_envs][H*ts][W*ts][3]. */
int32_t mg_render_frame(const MgConfig* cfg, const MgState* st, const int32_t* env_ids, int32_t n_envs,
                        const uint8_t* frame_atlas, int32_t frame_tile_size, int32_t highlight,
                        uint32_t frame_amax, uint8_t* out, void* stream);
/* frame_amax: the four per-dir max sprite alphas at frame_tile_size packed little-endian (only used
 * when prestige_mask != 0). */

/* LDS bytes per workgroup mg_render_obs needs for `cfg` in its smallest shape (4-wave workgroups, the
 * atlas read in place when it does not fit next to the per-env scratch).  More than 163840 (160 KiB,
 * gfx950): the launch would fail with MG_E_LAUNCH — hosts check this when they build the config
 * (no device access; obj / atlas may still be NULL). */
int32_t mg_render_obs_lds_bytes(const MgConfig* cfg);

/* Which instantiation of the observation kernel `cfg` gets from the launcher (mg_render_obs and mg_step_render launch the
 * same one), as rocprofv3 prints it: "mg::render_kernel<VS, TS, WPB, V, RM>" — view size, tile size (0: read from cfg at
 * run time), waves per workgroup, variant (0 plain, 8 atlas read in place, 9 'prestige' recolouring, 12 both), raster (0 by
 * tile size: 16-byte chunks at 8 / 16 / 32, assemble-and-stream otherwise; 2 gather).  No device access, nothing is launched
 * (obj / atlas may be NULL).  Returns a bit mask >= 0: 1 = the view size, 2 = the tile size is a run-time value — 3 is the
 * fully generic instantiation, 2-2.4x slower than a specialised one (hosts warn) — or MG_E_ARG / MG_E_LAUNCH (does not fit LDS). */
int32_t mg_render_kernel_name(const MgConfig* cfg, char* out, int32_t cap);

/* timing helper for bench.py: average duration (ms) of `iters` back-to-back mg_render_obs
 * launches on `stream`, bracketed by HIP events recorded on that same stream. */
int32_t mg_time_render_obs(const MgConfig* cfg, const MgState* st, uint8_t* obs, int32_t iters,
                           float* avg_ms, void* stream);

/* ---- memory helpers (optional: callers may bring any device-accessible memory) -------------------------------
 *
 * mg_host_flag_alloc: one int32 in pinned, coherent host memory, mapped into the device's address space:
 * *host is what the CPU reads, *dev is what goes into MgState.error_flag.  Zero-initialised. */
int32_t mg_host_flag_alloc(int32_t** host, int32_t** dev);
int32_t mg_host_flag_free(int32_t* host);

/* mg_obs_alloc / mg_obs_free: device memory straight from the driver (hipMalloc on `device`), outside any caching
 * allocator.  NULL on failure.  Nothing on the step path allocates: these are construction-time helpers, and any other
 * device memory is as valid an `obs` argument. */
void* mg_obs_alloc(uint64_t bytes, int32_t device);
int32_t mg_obs_free(void* ptr);

/* ---- where the observation buffers live ---------------------------------------------------------------------------
 *
 * MultiGridEnv's constructor allocates the observation arrays it returns (base.py:334-347, 453-474); for a batch they are
 * the one large output of a step, and WHERE in HBM they lie decides a fifth of the raster's speed (measured, MI355X,
 * profiles/r04/README.md section 1 + profiles/r05/README.md): the raster writes thousands of concurrent sequential
 * streams, and that pattern runs at 5.3 TB/s into a buffer that lies inside one of the driver's physical blocks, at the
 * speed of a dense fill (6.9 TB/s) into one that straddles the boundary between two blocks half and half — one valley per
 * allocation, at the block boundary, half a buffer wide on either side.  Nothing else moves it (stride, phase and number
 * of the streams, gaps, who writes what, address translation, L2 counters: all the same).
 *
 * mg_obs_place CONSTRUCTS `n_buffers` buffers on such boundaries for the launch configuration `cfg` (obs of
 * B * n_view-or-n_agents * P * P * 3 bytes each): a candidate is one hipMalloc of 3 P' bytes (P' = the power of two >= half
 * the buffer — the driver builds it from a 2 P' block and a P' block), the buffer the window centred on the junction;
 * candidates are timed with the raster itself (the state `st` as it is: HIP events around `iters` mg_render_obs launches on
 * `stream`, blocking) and kept alive until `n_buffers` of them run 12 % under the median candidate, then all the others
 * go back to the driver.  Buffers under 256 MiB are plain allocations (the effect needs thousands of streams), and so are
 * the buffers of a configuration whose raster writes them at under 3.5 TB/s (it is bound by something else than HBM).
 *   budget_bytes  bytes of candidates alive at any time; 0 = min(a quarter of the free memory, 32 GiB), raised to the kept
 *                 buffers + three first-level candidates while that is within half of the free memory (large buffers: a
 *                 16 GB buffer's candidates are 24 GiB each)
 *   seconds       time limit of a pass (not applied before the plain baseline allocations are in); <= 0 = 2 s, more for
 *                 candidates above 6 GiB (0.33 s per GiB of candidate, 12 s at most)
 *   flags         MG_PLACE_THOROUGH: larger block pairs (candidates of 6 P' and 12 P' bytes — a kept buffer then pins up
 *                 to 12x its size) and a second pass when the first found nothing; MG_PLACE_STIR: when nothing was found
 *                 and allocations were slow (memory nobody had before is cleared as it is handed out, front to back, all in
 *                 one block), one allocate-and-free of half the free memory (64 GiB at most) to mix the driver's free lists;
 *                 MG_PLACE_NO_REUSE: do not take released arenas (below)
 *   tuning        NULL, or overrides of the search's constants (tests force its later stages with them)
 *   out           [n_buffers] device pointers, 4 KiB-aligned, owned by the library: give each back with mg_obs_release
 *   stats         NULL, or what happened: found (0: no candidate was in the fast class — the best seen were kept, the caller
 *                 may try again later or with MG_PLACE_THOROUGH), kept_ms, pinned_bytes (what the kept buffers' allocations
 *                 hold: 1.5 .. 3 x the buffers at the default level) ...
 * Returns MG_OK, MG_E_ARG, MG_E_NOMEM (nothing handed out) or MG_E_LAUNCH.
 *
 * mg_obs_release gives a placed buffer back.  An arena of the fast class is REMEMBERED (per process and device; at most
 * min(8 GiB, a sixteenth of the device) of them): the next mg_obs_place of the same buffer size on that device takes it,
 * checks it with one measurement and does not search (stats->reused).  mg_obs_trim(device) (-1: every device) returns
 * the remembered arenas to the driver and reports how many there were.  This record is the library's only process state
 * (a mutex guards it); everything else in this header is re-entrant. */
#define MG_PLACE_MAX 8      /* buffers per call */
#define MG_PLACE_ALL 136    /* candidates recorded in MgPlaceStats.all_ms */
#define MG_PLACE_STIR 1
#define MG_PLACE_THOROUGH 2
#define MG_PLACE_NO_REUSE 4
#define MG_PLACE_STOP_FOUND 1   /* MgPlaceStats.stopped: the kept set is `gain` under the median candidate — or takes the raster's bytes
                                 * at 5.9 TB/s and more, the rate of the fast class (buffers of several GB: wherever they lie) */
#define MG_PLACE_STOP_CAP 2     /* max_candidates measured */
#define MG_PLACE_STOP_TIME 3
#define MG_PLACE_STOP_MEMORY 4  /* the budget does not hold another candidate (after the losers went back, up to six times) */
#define MG_PLACE_STOP_OOM 5     /* hipMalloc failed */
#define MG_PLACE_STOP_SMALL 6   /* buffers under min_bytes: plain allocations */
#define MG_PLACE_STOP_UNBOUND 7 /* the raster writes the plain buffers at under 3.5 TB/s: not bound by HBM writes, nothing to place */
typedef struct MgPlaceTuning {  /* 0 = the default of each */
    double gain;                /* 0.12 */
    double slow_alloc_s_per_gib;/* MG_PLACE_STIR only when allocations took at least this long: 0.02; < 0: always */
    uint64_t min_bytes;         /* 256 MiB */
    uint64_t stir_bytes;        /* cap of the allocate-and-free: 64 GiB */
    int32_t max_candidates;     /* per pass: 192 (the first MG_PLACE_ALL are recorded in MgPlaceStats.all_ms) */
    int32_t iters;              /* raster launches per measurement: 3 */
    int32_t share;              /* processes that share this device's memory (ranks of an oversubscribed launch): the default
                                 * budget is worked out from 1 / share of what is free.  0 / 1: this process counts on all of it */
    int32_t reserved1;
    double fast_rate;           /* bytes per second at which a kept set counts as found whatever the median says: 5.9e12; < 0: never */
} MgPlaceTuning;
typedef struct MgPlaceStats {
    int32_t found, reused, candidates, windows;   /* windows: positions measured (>= candidates) */
    int32_t passes, level, plain_stage, stopped;  /* level: the largest block pair tried (candidates of 3 P' << level) */
    float kept_ms[MG_PLACE_MAX];                  /* the raster into each kept buffer */
    float median_ms, reserved0;                   /* ... and into the median candidate */
    double seconds, alloc_seconds;                /* the whole call; inside hipMalloc */
    uint64_t buffer_bytes, candidate_bytes, alloc_bytes, pinned_bytes, stirred_bytes, budget_bytes;
    uint64_t window_offset[MG_PLACE_MAX];         /* of each kept buffer inside its allocation */
    uint64_t arena_bytes[MG_PLACE_MAX];           /* ... and that allocation's size */
    float all_ms[MG_PLACE_ALL];                   /* the first MG_PLACE_ALL candidates measured, in order (the first n_buffers: plain allocations) */
} MgPlaceStats;
int32_t mg_obs_place(const MgConfig* cfg, const MgState* st, int32_t n_buffers, uint64_t budget_bytes, double seconds,
                     int32_t flags, const MgPlaceTuning* tuning, void** out, MgPlaceStats* stats, void* stream);
int32_t mg_obs_release(void* ptr);
int32_t mg_obs_trim(int32_t device);

#ifdef __cplusplus
}
#endif
#endif
