/*
 * copycat_apply.h — C-ABI of the MI355X batched commit-apply engine.
 *
 * This is the drop-in boundary for ONE hot path of madjam/copycat (Atomix 0.1.0 on Copycat 1.0.0-beta4):
 * applying a batch of committed Raft log entries to many multiplexed resource state machines.
 * In the reference that path is, per committed entry, on one state-machine thread:
 *
 *   Copycat apply loop [not vendored]
 *     -> ResourceManager.operateResource           manager/src/main/java/io/atomix/manager/ResourceManager.java:56-72
 *     -> ResourceManagerStateMachineExecutor.execute manager/.../ResourceManagerStateMachineExecutor.java:90-102
 *     -> ResourceStateMachineExecutor.executeCommand resource/.../ResourceStateMachineExecutor.java:73-91
 *     -> AtomicValueState / MapState / LockState / LeaderElectionState / MembershipGroupState methods
 *
 * The engine replaces that chain for a whole batch: the host encodes the batch into the SoA columns of
 * cc_batch (one row per commit, in log order) and calls cc_apply_batch(); hand-written gfx950 kernels
 * produce one (status, value) row per commit plus an event stream.
 *
 * Conventions
 *  - Every call returns an int: CC_OK (0) or a negative CC_ERR_* code.  Per-commit failures (the Java
 *    exceptions) never fail the call: they are reported in the commit's status byte.
 *  - A handle is used from one host thread at a time (the reference applies on one thread too).
 *  - Pointers named d_* are device (HBM) pointers; h_* are host pointers.  `stream` is a hipStream_t
 *    passed as void* (NULL = the legacy default stream).  Device calls are stream-ordered and
 *    asynchronous; results are final after cc_sync() or a sync on the caller's stream.
 *  - No torch, no C++ types: plain C so that a JNI / Panama FFM / ctypes stub can bind it
 *    (INTEGRATION.md shows the bindings).
 */
#ifndef COPYCAT_APPLY_H
#define COPYCAT_APPLY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CC_ABI_VERSION 6

/* ---- return codes ------------------------------------------------------------------------------ */
#define CC_OK               0
#define CC_ERR_INVALID     -1  /* bad argument / handle */
#define CC_ERR_HIP         -2  /* HIP runtime error (message: cc_last_error) */
#define CC_ERR_CAPACITY    -3  /* batch / resource / instance / table capacity exceeded */
#define CC_ERR_UNSUPPORTED -4  /* an op or resource type this build does not run on the GPU */
#define CC_ERR_STATE       -5  /* engine state corrupt (a device-side check failed) */

/* ---- resource (state machine) types; ResourceManager.getResource instantiates one per key ----------
 * ResourceManager.java:92 `commit.operation().type().newInstance()`                                    */
#define CC_RES_NONE      0
#define CC_RES_VALUE     1  /* AtomicValueState  atomic/.../state/AtomicValueState.java:32 (also DistributedAtomicLong) */
#define CC_RES_MAP       2  /* MapState          collections/.../state/MapState.java:32 */
#define CC_RES_LOCK      3  /* LockState         coordination/.../state/LockState.java:33 */
#define CC_RES_ELECTION  4  /* LeaderElectionState coordination/.../state/LeaderElectionState.java:31 */
#define CC_RES_GROUP     5  /* MembershipGroupState coordination/.../state/MembershipGroupState.java:33 */
#define CC_RES_SET       6  /* SetState          collections/.../state/SetState.java:32 (shares the map table) */
#define CC_RES_QUEUE     7  /* QueueState        collections/.../state/QueueState.java:33 (a FIFO of CC_QUEUE_CAP) */
#define CC_RES_MULTIMAP  8  /* MultiMapState     collections/.../state/MultiMapState.java:30 (shares the map table) */
#define CC_RES_TOPIC     9  /* TopicState        coordination/.../state/TopicState.java:31 (listeners keyed by instance id) */
#define CC_RES_BUS      10  /* MessageBusState   coordination/.../state/MessageBusState.java:30 (members keyed by instance id +
                               topics -> registrations keyed by instance id, both in one coordination block) */
#define CC_QUEUE_CAP    64

/* ---- op codes = Catalyst @SerializeWith ids of the inner operation ------------- */
#define CC_OP_DELETE            1   /* ResourceStateMachine.DeleteCommand (no wire id) ResourceStateMachine.java:53 */
/* AtomicValueCommands.java:93-260 */
#define CC_OP_VALUE_GET        50   /* query */
#define CC_OP_VALUE_SET        51
#define CC_OP_VALUE_CAS        52   /* CompareAndSet(expect=a, update=b) */
#define CC_OP_VALUE_GETANDSET  53
#define CC_OP_VALUE_LISTEN     54
#define CC_OP_VALUE_UNLISTEN   55
/* MapCommands.java:134-450 */
#define CC_OP_MAP_CONTAINSKEY   60  /* query */
#define CC_OP_MAP_CONTAINSVALUE 61  /* query */
#define CC_OP_MAP_PUT           62
#define CC_OP_MAP_PUTIFABSENT   63
#define CC_OP_MAP_GET           64  /* query */
#define CC_OP_MAP_GETORDEFAULT  65  /* query */
#define CC_OP_MAP_REMOVE        66
#define CC_OP_MAP_REMOVEIFPRESENT 67
#define CC_OP_MAP_REPLACE       68
#define CC_OP_MAP_REPLACEIFPRESENT 69
#define CC_OP_MAP_ISEMPTY       70  /* query */
#define CC_OP_MAP_SIZE          71  /* query */
#define CC_OP_MAP_CLEAR         72
/* LeaderElectionCommands.java:80-99 */
/* QueueState (collections/.../state/QueueCommands.java:133-235): the element travels in operand a */
#define CC_OP_QUEUE_CONTAINS   90  /* query */
#define CC_OP_QUEUE_ADD        91
#define CC_OP_QUEUE_OFFER      92
#define CC_OP_QUEUE_PEEK       93  /* query */
#define CC_OP_QUEUE_POLL       94
#define CC_OP_QUEUE_ELEMENT    95
#define CC_OP_QUEUE_REMOVE     96  /* a = element, or NULL: remove the head */
#define CC_OP_QUEUE_SIZE       97  /* query */
#define CC_OP_QUEUE_ISEMPTY    98  /* query */
#define CC_OP_QUEUE_CLEAR      99
/* SetState (collections/.../state/SetCommands.java:133-238): the element travels in the key column (key tag in
 * CC_FLAGS), the ttl of Add in aux */
#define CC_OP_SET_CONTAINS     100  /* query */
#define CC_OP_SET_ADD          101
#define CC_OP_SET_REMOVE       102
#define CC_OP_SET_SIZE         103  /* query */
#define CC_OP_SET_ISEMPTY      104  /* query */
#define CC_OP_SET_CLEAR        105
/* MultiMapState (collections/.../state/MultiMapCommands.java:205-441): the key travels in the key column (key tag
 * in CC_FLAGS), the value in operand a, Put's ttl in aux.  ContainsEntry and ContainsValue have no handler in
 * MultiMapState (unknown operation).  MultiMapState.put never stores its value (:76-82): the state is the set of
 * keys put and not removed since; every Put commit stays retained (never cleaned or closed).               */
#define CC_OP_MMAP_CONTAINSKEY   75  /* query */
#define CC_OP_MMAP_CONTAINSENTRY 76  /* query (no handler) */
#define CC_OP_MMAP_CONTAINSVALUE 77  /* query (no handler) */
#define CC_OP_MMAP_PUT           78
#define CC_OP_MMAP_GET           79  /* query */
#define CC_OP_MMAP_REMOVE        80  /* a = value, or NULL: remove the key */
#define CC_OP_MMAP_REMOVEVALUE   81  /* a = value */
#define CC_OP_MMAP_ISEMPTY       82  /* query */
#define CC_OP_MMAP_SIZE          83  /* query */
#define CC_OP_MMAP_CLEAR         84

#define CC_OP_ELECT_LISTEN     110
#define CC_OP_ELECT_UNLISTEN   111
#define CC_OP_ELECT_ISLEADER   112  /* query */
/* LockCommands.java:59-93 */
#define CC_OP_LOCK_LOCK        115
#define CC_OP_LOCK_UNLOCK      116
/* MembershipGroupCommands.java:62-140 */
#define CC_OP_GROUP_JOIN       120
#define CC_OP_GROUP_LEAVE      121
#define CC_OP_GROUP_SCHEDULE   122
#define CC_OP_GROUP_EXECUTE    123
/* TopicCommands.java:53,64,80 (Publish: the message in operand a, its tag in CC_FLAGS) */
#define CC_OP_TOPIC_LISTEN     125
#define CC_OP_TOPIC_UNLISTEN   126
#define CC_OP_TOPIC_PUBLISH    127
/* MessageBusCommands.java (Join: the member's address in operand a; Register / Unregister: the topic in operand a;
 * both CC_TAG_HANDLE and below 2^CC_BUS_HANDLE_BITS, else the call fails with CC_ERR_UNSUPPORTED; 89 is ConsumerInfo,
 * not an op) */
#define CC_OP_BUS_JOIN         85
#define CC_OP_BUS_LEAVE        86
#define CC_OP_BUS_REGISTER     87
#define CC_OP_BUS_UNREGISTER   88
#define CC_BUS_HANDLE_BITS     32  /* a ConsumerInfo(topic, address) travels as one payload: topic << 32 | address */

/* ---- canonical tagged values: Java equals == (tag, payload) equality ---------- */
#define CC_TAG_NULL    0
#define CC_TAG_LONG    1   /* java.lang.Long, payload = two's complement i64 */
#define CC_TAG_INT     2   /* java.lang.Integer, payload = sign-extended i32 */
#define CC_TAG_BOOL    3   /* java.lang.Boolean, payload 0/1 */
#define CC_TAG_HANDLE  4   /* host-interned object (String, Runnable callback ...) */
#define CC_TAG_SET     5   /* result only: Set<Long> of MembershipGroupState.join; payload = member count,
                              members are written to the aux-result stream */
#define CC_TAG_MAP     7   /* result only: Map<String, Set<Address>> of MessageBusState.join; payload = topic count,
                              the rows follow in the event stream (CC_EV_BUS_TOPIC / CC_EV_BUS_ADDRESS) */
#define CC_TAG_LIST    6   /* result only: a Collection (MultiMapState get / remove(key)); payload = element count */

/* flags column: bits 0-2 tag(a), bits 3-5 tag(b), bits 6-7 key tag (keys are never null,
 * KeyCommand asserts notNull MapCommands.java:77): 0 LONG, 1 INT, 2 BOOL, 3 HANDLE.               */
#define CC_FLAGS(tag_a, tag_b, ktag) ((uint8_t)(((tag_a) & 7u) | (((tag_b) & 7u) << 3) | (((ktag) & 3u) << 6)))
#define CC_FLAG_TAG_A(f) ((f) & 7u)
#define CC_FLAG_TAG_B(f) (((f) >> 3) & 7u)
#define CC_FLAG_KTAG(f)  (((f) >> 6) & 3u)

/* ---- per-commit status (the Java exception class) ----------------------------------
 * status byte = code | (result tag << 4)                                                          */
#define CC_ST_OK               0
#define CC_ST_UNKNOWN_SESSION  1  /* ResourceManagerException "unknown resource session" ResourceManager.java:65 */
#define CC_ST_UNKNOWN_OP       2  /* IllegalStateException "unknown operation type" ResourceStateMachineExecutor.java:78 */
#define CC_ST_ILLEGAL_STATE    3  /* IllegalStateException "not the lock holder" LockState.java:70 */
#define CC_ST_ILLEGAL_ARGUMENT 4  /* IllegalArgumentException "unknown member" MembershipGroupState.java:89,112 */
#define CC_ST_NULL_POINTER     5  /* NullPointerException in MapState.containsValue MapState.java:52 */
#define CC_ST_TYPE_MISMATCH    6  /* ResourceManagerException "inconsistent resource type" ResourceManager.java:120,181 */
#define CC_ST_UNKNOWN_RESOURCE 7  /* ResourceManagerException "unknown resource" ResourceManager.java:216 */
#define CC_ST_NO_SUCH_ELEMENT  8  /* NoSuchElementException of ArrayDeque.element/remove() QueueState.java:113,144 */
#define CC_STATUS(code, tag)   ((uint8_t)(((code) & 15u) | (((tag) & 15u) << 4)))
#define CC_STATUS_CODE(s)      ((s) & 15u)
#define CC_STATUS_TAG(s)       (((s) >> 4) & 15u)

/* ---- event codes: Session.publish(event, msg) -> InstanceEvent{instance, msg}
 * ManagedResourceSession.java:64-71, InstanceEvent.java:29-80                                     */
#define CC_EV_CHANGE   1  /* AtomicValueState.change  AtomicValueState.java:68-72 */
#define CC_EV_LOCK     2  /* LockState "lock" true/false LockState.java:44,47,79 */
#define CC_EV_ELECT    3  /* LeaderElectionState "elect"(epoch=leader index) LeaderElectionState.java:44,60,80 */
#define CC_EV_JOIN     4  /* MembershipGroupState "join"(instance) :55 */
#define CC_EV_LEAVE    5  /* MembershipGroupState "leave"(instance) :40,75 */
#define CC_EV_EXECUTE  6  /* MembershipGroupState "execute"(callback) :95,115 */
#define CC_EV_MEMBER   7  /* not an event: one row per member of a join's Set<Long> result (ascending ids,
                             target = the joining instance, src CC_EVSRC_RESULT) MembershipGroupState.java:63 */
#define CC_EV_MESSAGE  8  /* TopicState "message"(message) TopicState.java:67-82: one per listener of the topic at the
                             publish row, target = the listener's instance slot, src CC_EVSRC_COMMIT, tag / payload =
                             the canonical message (payload 0 for NULL); within one publish in ascending listener
                             instance id (engine-defined: each goes to a different session) */
#define CC_EV_BUS_LEAVE      9  /* MessageBusState.close :35-40 "leave"(closed instance id, tag LONG) to every remaining
                                  member, src CC_EVSRC_CLOSE, whether or not the closed instance was a member */
#define CC_EV_BUS_REGISTER  10  /* "register"(ConsumerInfo) :112-114 to every member; tag HANDLE, payload = topic << 32 |
                                  address of the registrant; src CC_EVSRC_COMMIT, ascending member instance id */
#define CC_EV_BUS_UNREGISTER 11 /* "unregister"(ConsumerInfo) :84-86,134-136, same layout; a leave publishes one fan-out
                                  per topic of the leaver, in ascending topic handle (engine-defined) */
#define CC_EV_BUS_TOPIC     12  /* not an event: a row of a join's Map result (src CC_EVSRC_RESULT, target = the joiner):
                                  payload = a topic handle, ascending; followed by its CC_EV_BUS_ADDRESS rows */
#define CC_EV_BUS_ADDRESS   13  /* not an event: one distinct address of the topic row before it, ascending (none: an
                                  empty set) */

/* event source */
#define CC_EVSRC_COMMIT 0  /* published while applying commit `pos` */
#define CC_EVSRC_TIMER  1  /* published by a timer that fired at commit `pos` */
#define CC_EVSRC_CLOSE  2  /* published by a session close/expire fan-out */
#define CC_EVSRC_RESULT 3  /* a variable-length result row (CC_EV_MEMBER) */

/* ---- engine configuration ------------------------------------------------------------------------ */
typedef struct cc_config {
  uint32_t max_resources;   /* resource slots (ResourceManager.resources), <= 131072            */
  uint32_t max_instances;   /* instance-session slots (ResourceManager.sessions)               */
  uint64_t max_batch;       /* max commits per cc_apply_batch call                               */
  uint64_t max_events;      /* capacity of the device event stream per batch                      */
  uint64_t map_capacity;    /* live map entries across all CC_RES_MAP resources (0 = no maps; at most
                               2M: the table has 2^k regions of 2048 entries, >= 2 x map_capacity) */
  int32_t  device;          /* HIP device ordinal                                                  */
  uint32_t flags;           /* CC_CFG_* */
  uint64_t sub_batch;       /* commits per internal sub-batch (0 = default 24Mi; rounded up to a multiple
                               of 16384, at most 24Mi; an engine with maps, coordination resources or
                               value events runs its batches in sub-batches of at most 16Mi)        */
  uint32_t coord_cap;       /* entries per coordination resource: lock waiters, election listeners, group
                               members, value listeners, queue elements (0 = 64 = CC_LOCK_QUEUE; else a power
                               of two in [64, 65536]; CC_ERR_CAPACITY beyond).  Device memory per resource slot:
                               32 + 24 x coord_cap bytes; entries past the first 8 are walked in global memory. */
  uint32_t reserved32;
  uint64_t reserved[3];
} cc_config;

#define CC_CFG_TIMERS_DEFERRED 1u  /* manager-mode timer order (A8): due timers fire after the commit
                                      that advanced time (ResourceManagerStateMachineExecutor.java:104-109) */
#define CC_CFG_VALUE_RETAINED  4u  /* keep, per AtomicValue slot, the log index of the commit the state machine
                                      still retains (`current`, never clean()ed): cc_read_value_retained  */
#define CC_CFG_VALUE_EVENTS    2u  /* AtomicValue Listen/Unlisten + "change" events on the GPU (every value
                                      resource then runs on the event-capable kernel)              */

/* Coordination resources (lock / election / group / queue) keep their variable-size state in per-resource
 * blocks of cc_config.coord_cap entries; the defaults (coord_cap = 0): at most CC_LOCK_QUEUE waiters per lock,
 * CC_ELECTION_LISTENERS listeners per election, CC_GROUP_MEMBERS members per group, CC_VALUE_LISTENERS listeners per
 * value, CC_QUEUE_CAP elements per queue (CC_ERR_CAPACITY beyond).
 * The time column must be non-decreasing within a batch when lock timeouts are used (Raft log time).   */
#define CC_LOCK_QUEUE          64
#define CC_ELECTION_LISTENERS  64
#define CC_GROUP_MEMBERS       64
#define CC_VALUE_LISTENERS     64
#define CC_TOPIC_LISTENERS     64  /* coord_cap listeners per topic; at coord_cap 65536 the limit is 65,535 (a commit's
                                      event count is 16 bits) */
#define CC_BUS_ENTRIES         64  /* coord_cap entries per bus in all: members + registrations + empty-topic markers;
                                      an entry is also refused when max(members, 2) x registrations would pass 65,535
                                      (a commit's event count is 16 bits; binds only at coord_cap >= 512) */

/* ---- one batch of committed entries, SoA, log order ------------------------------------------------
 * Row i is InstanceCommand/InstanceQuery{instance, op} of log entry index[i]
 * (InstanceOperation.java:59-69; ResourceManagerCommit.index/time ResourceManagerCommit.java:54-66).
 * Columns an op does not use may hold anything; pointers of columns no op in the batch uses may be NULL.
 * The columns each op reads (`a` implies tag a of the flags byte, `b` tag b, `key` the key tag; an unused tag field may
 * hold any bits, the result-only tags 5..7 and an unregistered HANDLE key tag included):
 *
 *   key a b aux | MAP_REPLACEIFPRESENT
 *   key a aux   | MAP_PUT, MAP_PUTIFABSENT, MAP_REPLACE, MMAP_PUT, GROUP_SCHEDULE
 *   key a       | MAP_GETORDEFAULT, MAP_REMOVEIFPRESENT, MMAP_CONTAINSENTRY, MMAP_REMOVE, GROUP_EXECUTE
 *   key aux     | SET_ADD
 *   key         | MAP_CONTAINSKEY, MAP_GET, MAP_REMOVE, MMAP_CONTAINSKEY, MMAP_GET, MMAP_SIZE, SET_CONTAINS, SET_REMOVE
 *   a b         | VALUE_CAS
 *   a           | VALUE_SET, VALUE_GETANDSET, MAP_CONTAINSVALUE, MMAP_CONTAINSVALUE, MMAP_REMOVEVALUE, QUEUE_CONTAINS,
 *                 QUEUE_ADD, QUEUE_OFFER, QUEUE_REMOVE, TOPIC_PUBLISH, BUS_JOIN, BUS_REGISTER, BUS_UNREGISTER
 *   aux         | LOCK_LOCK
 *
 * Every other op byte reads nothing; index, time, inst and op are always read.  The op decides, not the resource it
 * lands on: a MAP_PUT on a lock is an unknown operation whatever its columns hold.  (tests/abi_cases.py USED is the
 * same table; tests/test_gpu_dont_care.py and tests/test_gpu_op_matrix.py hold the engine to it.) */
typedef struct cc_batch {
  const uint64_t* index;  /* log index (Commit.index())                                         */
  const uint64_t* time;   /* log time, ms (Commit.time()); drives TTL / timeout timers           */
  const uint32_t* inst;   /* instance-session slot (InstanceOperation.resource -> sessions map)  */
  const uint8_t*  op;     /* CC_OP_*                                                              */
  const uint8_t*  flags;  /* CC_FLAGS(tag a, tag b, key tag)                                      */
  const uint64_t* key;    /* map key / group member instance slot                                 */
  const uint64_t* a;      /* value / expect / default-less operand                                */
  const uint64_t* b;      /* update / replace / default operand                                   */
  const uint64_t* aux;    /* ttl / lock timeout / schedule delay (signed i64)                     */
} cc_batch;

/* per-commit results (caller-allocated, n rows) */
typedef struct cc_results {
  uint8_t*  status;       /* CC_STATUS(code, result tag) */
  uint64_t* value;        /* result payload                */
} cc_results;

/* event stream (caller-allocated, capacity rows); count written to *count (device u64) */
typedef struct cc_events {
  uint32_t* pos;          /* batch row that produced the event                          */
  uint32_t* target;       /* instance slot whose session receives it                    */
  uint8_t*  code;         /* CC_EV_*                                                     */
  uint8_t*  src;          /* CC_EVSRC_*                                                  */
  uint8_t*  tag;          /* payload tag                                                 */
  uint64_t* payload;
  uint64_t  capacity;
  uint64_t* count;        /* device pointer: number of events written (may exceed capacity:
                             then the call returns CC_ERR_CAPACITY on sync)                */
} cc_events;

typedef struct cc_engine cc_engine;

/* ---- lifecycle ------------------------------------------------------------------------------------ */
int  cc_abi_version(void);
const char* cc_last_error(void);
/* ResourceManager constructor + StateMachine.configure (ResourceManager.java:35-50) */
int  cc_engine_create(const cc_config* cfg, cc_engine** out);
int  cc_engine_destroy(cc_engine* e);
int  cc_sync(cc_engine* e);
/* The engine's stream (hipStream_t as void*). */
void* cc_engine_stream(cc_engine* e);

/* ---- resource and instance registry (host-side control commands) --------------------------------
 * New resource: ResourceManager.getResource/createResource new-key branch (ResourceManager.java:84-100,157-176);
 * the engine allocates state for `slot` (chosen by the host: resource id -> dense slot).       */
int  cc_resource_create(cc_engine* e, uint32_t slot, uint32_t type);
/* Bulk form: slots [first, first+count) all of `type`. */
int  cc_resource_create_range(cc_engine* e, uint32_t first, uint32_t count, uint32_t type);
/* ResourceManager.deleteResource (ResourceManager.java:212-235): delete() state, cancel timers,
 * and close every instance slot registered to the resource.                                   */
int  cc_resource_delete(cc_engine* e, uint32_t slot);
/* A ManagedResourceSession (ResourceManager.java:103-106,128-131,189-190): instance slot -> resource slot,
 * owned by client session `client_session`; `instance_id` is the Java instance id (= creating commit index). */
int  cc_instance_open(cc_engine* e, uint32_t inst, uint32_t res_slot, uint64_t instance_id, uint64_t client_session);
/* Bulk form: instance slot first+k -> resource slot res_first+k, instance id id_first+k, one client session. */
int  cc_instance_open_range(cc_engine* e, uint32_t first, uint32_t count, uint32_t res_first, uint64_t id_first,
                            uint64_t client_session);

/* ---- ResourceManager control commands (ResourceManager.java:77-235) ------------------------------------
 * GetResource / CreateResource / DeleteResource / ResourceExists commits, applied by the host between batches in log
 * order (manager.hip).  `key` is the host-interned GetResource.key String, `client` = commit.session().id(),
 * `index` = commit.index().  Resource ids and instance ids are commit indices; the engine picks the slots.
 * *status = CC_STATUS(CC_ST_OK, CC_TAG_LONG) with *instance_id = the ManagedResourceSession id (the Long the reference
 * returns) and *inst_slot = the instance slot its commits carry in cc_batch.inst; or CC_ST_TYPE_MISMATCH
 * ("inconsistent resource type" :119-121,178-181).  Return codes: CC_ERR_CAPACITY when no slot is free.       */
/* getResource :77-143 — a new key creates the resource (id = index); a client that already holds an instance of
 * the resource gets that instance back (ResourceHolder.sessions :137-141) */
int  cc_get_resource(cc_engine* e, uint64_t key, uint32_t type, uint64_t client, uint64_t index, uint64_t* instance_id,
                     uint32_t* inst_slot, uint8_t* status);
/* createResource :148-196 — always a new instance (id = index), not recorded in ResourceHolder.sessions */
int  cc_create_resource(cc_engine* e, uint64_t key, uint32_t type, uint64_t client, uint64_t index, uint64_t* instance_id,
                        uint32_t* inst_slot, uint8_t* status);
/* resourceExists :201-207 */
int  cc_resource_exists(cc_engine* e, uint64_t key, uint8_t* exists);
/* deleteResource :212-235 by RESOURCE id (clients send their instance id, so only the creating instance matches,
 * A13): *status = OK|BOOL (true), CC_ST_UNKNOWN_RESOURCE, or CC_ST_ILLEGAL_STATE when the state machine's delete()
 * throws (a lock / election whose holder commit was already cleaned): the resource then leaves `resources` but its
 * key and instances stay, and commits on those instances get CC_ST_NULL_POINTER (:62,71).                     */
int  cc_delete_resource(cc_engine* e, uint64_t resource_id, uint8_t* status);
/* id -> slot lookups of ResourceManager.sessions / resources (-1: none) */
int  cc_instance_slot(cc_engine* e, uint64_t instance_id, int64_t* slot);
int  cc_resource_slot(cc_engine* e, uint64_t resource_id, int64_t* slot);

/* java.lang.String.hashCode of HANDLE keys.  A HANDLE key is a host-interned String (GetResource / DistributedMap keys
 * are Strings); java.util.HashMap places it by String.hashCode, which the handle alone does not give.  Map resources
 * need it to answer containsValue in the reference's iteration order (MapState.java:49-60 walks map.values()) and
 * to follow the table's capacity exactly (HashMap.treeifyBin resizes a table below capacity 64 when one bin reaches 9
 * keys).  cc_wire_decode registers the Strings it interns itself; a host that interns Strings on its own registers
 * them here before the batch that uses them (a map operation that needs an unregistered key's hash fails the batch
 * with CC_ERR_STATE).  Registering a handle again with another hash is CC_ERR_INVALID. */
int  cc_handle_hashes(cc_engine* e, const uint64_t* h_handles, const int32_t* h_hashes, uint64_t count);

/* ---- the hot path --------------------------------------------------------------------------------
 * Apply n committed entries (device-resident columns) in log order.  Replaces the per-entry chain
 * ResourceManager.operateResource (ResourceManager.java:56-72) -> executors -> state machine method.
 * `events` may be NULL when no op in the batch publishes (then publishing ops fail with CC_ERR_UNSUPPORTED). */
/* Map containsValue/size/isEmpty/clear/Delete rows (MapState.java:49-60,233-274) read or reset a whole map: on
 * an engine with maps the call first scans the batch for them (one host sync), then applies the rows between
 * them as segments and each such row against the table as it stands at its log position.  A containsValue whose
 * answer depends on java.util.HashMap iteration order when the map's table capacity is not determined exactly
 * fails the batch with CC_ERR_STATE (see copycat_amd/csrc/map_wide.hip). */
/* d_out->status must be 4-byte aligned and d_out->value 16-byte aligned (hipMalloc / torch allocations are). */
int  cc_apply_batch(cc_engine* e, const cc_batch* d_cols, uint64_t n, const cc_results* d_out,
                    const cc_events* d_events, void* stream);
/* ---- host-memory entry points (copycat_amd/csrc/host_path.hip) -------------------------------------------------
 * For a host that holds no device pointers (a JVM through Panama FFM / JNI): host columns in,
 * host results and events out.  The engine stages them in device buffers it owns (grown on demand, kept between
 * calls); every call is synchronous.  A host event stream is a cc_events whose column pointers AND `count` point to
 * host memory: *count = the events published (when it exceeds `capacity` the call returns CC_ERR_CAPACITY after
 * copying the first `capacity` rows).  Events reach the client as Session.publish -> InstanceEvent{instance, msg}
 * (ManagedResourceSession.java:64-71, InstanceEvent.java:29-80): `target` is the instance slot whose session
 * receives the event, rows in publish order (log row, then the state machine's publish order). */
/* Host columns/results: H2D, apply, D2H, sync (PCIe-inclusive path).  Publishing ops fail with
 * CC_ERR_UNSUPPORTED here: use cc_apply_batch_host_events. */
int  cc_apply_batch_host(cc_engine* e, const cc_batch* h_cols, uint64_t n, const cc_results* h_out);
/* The same with the event stream (lock grants, elections, joins / leaves, executes, value changes). */
int  cc_apply_batch_host_events(cc_engine* e, const cc_batch* h_cols, uint64_t n, const cc_results* h_out,
                                const cc_events* h_events);
/* Highest log index applied so far (the applied watermark; all-gathered across GPUs by the host). */
int  cc_applied_index(cc_engine* e, uint64_t* out);
/* Cumulative path counters of the engine (observability; ABI 5): out[0] whole-map / schedule rows applied as batch
 * barriers, out[1] map containsValue rows answered in the stream (map_cv.hip), out[2] sub-batches launched,
 * out[3] map events sorted and replayed (small maps' HashMap models, size rows, cleared maps' sizes: map_small.hip),
 * out[4] big HashMap models held now (maps past capacity 64 with a tree bin: map_big.hip; reading it syncs).
 * n = entries of `out` to fill (at most 5). */
int  cc_engine_counters(cc_engine* e, uint64_t* out, uint32_t n);
/* The group / segment arithmetic of the value-only apply (host arithmetic, no device needed; symbols added under the
 * unchanged CC_ABI_VERSION 6).  A value-only call longer than a sub-batch is partitioned and unpermuted once per
 * *group* and applied once per *segment* (= sub-batch) of the group.
 *   cc_value_group_knob     the text of the environment variable CC_VALUE_GROUP_TILES (read when an engine is created):
 *                           NULL / "" -> UINT64_MAX (groups as large as the kernels' 32-bit staging offsets allow:
 *                           2^29 - 4096 positions, in whole segments), "0" -> 0 (one partition and one unpermute per
 *                           sub-batch), "k" -> at most k tiles of 8192 rows per group, rounded down to whole segments
 *                           (at least one); anything else CC_ERR_INVALID.
 *   cc_value_group_plan     out[0] rows per group at most (0: the per-sub-batch path), out[1] groups a call of n rows
 *                           runs, out[2] staging positions allocated for it (min(n, max_batch, out[0]) in whole tiles).
 *   cc_value_group_segment  segment j of a group of `rows` rows staged in arrays of staging_rows positions: out[0] its
 *                           first row (from the group's first), out[1] rows, out[2] first tile, out[3] tiles, out[4]
 *                           its first dummy position counted from its first tile.  CC_ERR_CAPACITY when the group does
 *                           not fit the staging or the dummy rows would pass 2^29 positions; CC_ERR_INVALID for j past
 *                           the group's last segment. */
int  cc_value_group_knob(const char* text, uint64_t* tiles);
int  cc_value_group_plan(uint64_t n, uint64_t sub_batch, uint64_t max_batch, uint64_t knob_tiles, uint64_t* out /*[3]*/);
int  cc_value_group_segment(uint64_t rows, uint64_t sub_batch, uint64_t staging_rows, uint64_t j, uint64_t* out /*[5]*/);
/* The same watermark written stream-ordered into device memory (u64 at d_out) without a host sync: what a rank feeds
 * to the RCCL all-gather of applied watermarks after each batch. */
int  cc_applied_index_async(cc_engine* e, uint64_t* d_out, void* stream);

/* ---- snapshot / restore ---------------------------------------------------------------------------
 * Replaces recovery by full log replay (the reference replays Copycat's log, AbstractReplicaTest.java:82-84):
 * the engine's whole device state plus its host registry mirrors, as one host buffer.  Save syncs first;
 * cc_snapshot_restore needs an engine created with the same max_resources, max_instances, map_capacity (the same
 * table: the same number of 2,048-entry regions) and coord_cap; cc_snapshot_restore_grow (below) takes an engine
 * whose map_capacity and coord_cap are the same or larger. */
int  cc_snapshot_size(cc_engine* e, uint64_t* bytes);
int  cc_snapshot_save(cc_engine* e, void* h_buf, uint64_t cap);
int  cc_snapshot_restore(cc_engine* e, const void* h_buf, uint64_t size);

/* ---- restore into an engine with larger capacities --------------------------------------------------
 * The engine's collections are fixed at creation (coord_cap entries per coordination block, map_capacity live map / set
 * / multimap entries); the reference's are unbounded.  When a prefix apply (cc_apply_batch_host_prefix,
 * cc_apply_batch_prefix) stops before a commit that a full block or table region cannot hold, the host saves a
 * snapshot, reads what it was taken from (cc_snapshot_info), creates an engine with a larger coord_cap and / or
 * map_capacity, restores into it with cc_snapshot_restore_grow and resumes at the stopped row: no commit fails that the
 * reference would have applied.
 *
 * cc_snapshot_info reads the snapshot's header only: no engine, no HIP call.  map_capacity is the largest
 * cc_config.map_capacity that gives the snapshot's table (table entries / 2; 0: no maps).  CC_ERR_INVALID on a NULL
 * argument, a buffer shorter than the header, or a buffer that is no snapshot of this ABI.
 *
 * cc_snapshot_restore_grow accepts a snapshot whose max_resources, max_instances and CC_CFG_VALUE_RETAINED equal the
 * engine's, with coord_cap <= the engine's and a map table no larger than the engine's.  A snapshot without maps
 * restores into an engine with maps as an empty table; the reverse, and any shrink, is CC_ERR_INVALID.  Everything
 * cc_snapshot_restore validates is validated the same way and before any engine state changes (a refused call leaves
 * the engine as it was), and the staging memory is allocated before the first store into engine state.  When nothing
 * grows the call is cc_snapshot_restore.
 *
 * Afterwards the engine behaves as the snapshot's engine would have, with more room: every cc_read_* reader,
 * cc_retained_bitmap and cc_applied_index report what the source engine reported, and every later apply gives the
 * results, events and state the reference gives.  No per-map model moves (sizes, HashMap capacity levels, the small and
 * big models, the peak and drop counters, generations, the compacted-key set's membership).  Positions inside the map
 * table are no part of the contract.  A snapshot saved from the grown engine is an ordinary snapshot of the new
 * configuration (cc_snapshot_restore takes it).  The sections that change shape (the map table's columns, the
 * compacted-key set, the coordination blocks) are migrated on the device (grow.hip).
 *
 * cc_snapshot_grow_timing(enable, ms): diagnostics.  Copies the calling thread's last cc_snapshot_restore_grow's
 * kernel times to ms[0..2] (milliseconds: table, compacted-key set, coordination blocks; 0 for a kernel that did not
 * run; ms may be NULL), then switches the timing on or off for that thread's next calls (on: the call waits after each
 * kernel).  These calls exist from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added). */
#define CC_SNAP_COORD           1u  /* cc_snapshot_info_t.flags: the snapshot holds coordination blocks */
#define CC_SNAP_TTL             2u  /*   its maps were in TTL mode */
#define CC_SNAP_VALUE_RETAINED  4u  /*   its engine was created with CC_CFG_VALUE_RETAINED */
typedef struct cc_snapshot_info_t {   /* what a snapshot was taken from */
  uint32_t max_resources, max_instances;
  uint64_t map_capacity;
  uint32_t coord_cap, flags;
  uint64_t applied;
} cc_snapshot_info_t;
int  cc_snapshot_info(const void* h_buf, uint64_t size, cc_snapshot_info_t* out);
int  cc_snapshot_restore_grow(cc_engine* e, const void* h_buf, uint64_t size);
int  cc_snapshot_grow_timing(int enable, float* ms);

/* ---- state readback for parity checks ------------------------------------------------------------ */
/* AtomicValueState {value, current != null} for slots [first, first+count) (AtomicValueState.java:34-35) */
int  cc_read_value_state(cc_engine* e, uint32_t first, uint32_t count, uint8_t* h_tag, uint64_t* h_value,
                         uint8_t* h_has_current);
/* Log compaction (Commit.clean(), AtomicValueState.java:88-157): per value slot in [first, first+count), the
 * index of the one commit still retained (`current`), 0 if none.  Needs CC_CFG_VALUE_RETAINED.          */
int  cc_read_value_retained(cc_engine* e, uint32_t first, uint32_t count, uint64_t* h_index);
/* MapState.map of one map slot (MapState.java:33): *count = live entries; the first min(cap, count), sorted
 * by (key tag, key), go to the arrays (key tag as a CC_TAG_*; commit_index may be NULL).               */
int  cc_read_map_entries(cc_engine* e, uint32_t slot, uint64_t cap, uint64_t* count, uint8_t* h_key_tag, uint64_t* h_key,
                         uint8_t* h_value_tag, uint64_t* h_value, uint64_t* h_commit_index);
/* Every map / set slot's live entries in one pass over the table (bulk form of cc_read_map_entries): *count =
 * entries; the first min(cap, count), sorted by (slot, key tag, key), go to the arrays.                      */
int  cc_read_map_table(cc_engine* e, uint64_t cap, uint64_t* count, uint32_t* h_slot, uint8_t* h_key_tag, uint64_t* h_key,
                       uint8_t* h_value_tag, uint64_t* h_value, uint64_t* h_commit_index);

/* LockState (LockState.java:33-36) after the timers due at the engine clock: holder instance slot (-1 none),
 * its commit index and cleaned flag; *count = queued waiters, the first min(cap, count) to the arrays. */
int  cc_read_lock_state(cc_engine* e, uint32_t slot, int64_t* holder, uint64_t* holder_index, uint8_t* holder_cleaned,
                        uint64_t cap, uint64_t* count, uint32_t* h_queue_inst, uint64_t* h_queue_index);
/* LeaderElectionState (LeaderElectionState.java:31-33): leader instance slot (-1 none) + index, listeners in
 * insertion order. */
int  cc_read_election_state(cc_engine* e, uint32_t slot, int64_t* leader, uint64_t* leader_index, uint64_t cap,
                            uint64_t* count, uint32_t* h_listener_inst, uint64_t* h_listener_index);
/* MembershipGroupState.members (MembershipGroupState.java:33): member instance ids, ascending. */
int  cc_read_group_members(cc_engine* e, uint32_t slot, uint64_t cap, uint64_t* count, uint64_t* h_ids);
/* TopicState.listeners (TopicState.java:32): listener instance ids, ascending, and each listener's Listen commit
 * index.  Exists from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added). */
int  cc_read_topic_listeners(cc_engine* e, uint32_t slot, uint64_t cap, uint64_t* count, uint64_t* h_ids,
                             uint64_t* h_index);
/* MessageBusState.members (MessageBusState.java:31): ascending instance id; each member's address handle, Join commit
 * index and whether delete() cleaned that commit (:148: the member stays a member).  Any array may be NULL. */
int  cc_read_bus_members(cc_engine* e, uint32_t slot, uint64_t cap, uint64_t* count, uint64_t* h_ids, uint64_t* h_addr,
                         uint64_t* h_index, uint8_t* h_cleaned);
/* MessageBusState.topics (:32): ascending (topic handle, instance id) with each Register commit index; a topic whose
 * registration map is empty is one row with id 0 and index 0.  Both exist from this commit on, ABI version unchanged. */
int  cc_read_bus_registrations(cc_engine* e, uint32_t slot, uint64_t cap, uint64_t* count, uint64_t* h_topic,
                               uint64_t* h_ids, uint64_t* h_index);
/* Log compaction for every state machine (Commit.clean()): the log indices of every commit
 * the slot's state machine still holds without having clean()ed it, ascending — *count of them, the first
 * min(cap, count) to h_index.  Value: `current` + listeners (AtomicValueState.java:41-157, needs
 * CC_CFG_VALUE_RETAINED); map / set: each entry's commit (MapState.java:279-287); lock: the holder unless
 * delete() cleaned it + waiters (LockState.java:41-98); election: the leader unless cleaned + listeners
 * (LeaderElectionState.java:35-108); group: members + pending schedule commits (MembershipGroupState.java:47-103);
 * queue: elements less the head element() cleaned (QueueState.java:51-199).  Plus the commits those state
 * machines drop without clean() — a listen that replaces a session's listener (AtomicValueState.java:41-49), a
 * member removed by close (MembershipGroupState.java:36-42) — which the log can never compact.            */
int  cc_read_retained(cc_engine* e, uint32_t slot, uint64_t cap, uint64_t* count, uint64_t* h_index);
/* Bulk compaction feed: bit (i - first) of d_bitmap (ceil(count / 64) u64 words in HBM, LSB first) is set iff
 * log index i in [first, first + count) is held by some resource's state machine without clean() -- the union over
 * every live resource slot of cc_read_retained, built on the device in one pass (retained.hip).  *h_count (may be
 * NULL) = the retained commits in the range.  A compactor calls it after a batch over (last compacted, commit index]:
 * clear bits are compactable (Commit.clean(), ResourceManagerCommit.java:79-81); a bit that cleared since the
 * previous call was released by a clean() in between.  Value resources need CC_CFG_VALUE_RETAINED.  Synchronous. */
int  cc_retained_bitmap(cc_engine* e, uint64_t first, uint64_t count, uint64_t* d_bitmap, uint64_t* h_count);
/* The same bitmap into host memory (ceil(count / 64) u64 words). */
int  cc_retained_bitmap_host(cc_engine* e, uint64_t first, uint64_t count, uint64_t* h_bitmap, uint64_t* h_count);
/* Log time advanced without a commit (ResourceManagerStateMachineExecutor timers): due lock
 * timeouts take effect (they publish nothing, LockState.java:54-58). */
int  cc_advance_time(cc_engine* e, uint64_t now);
/* Same, publishing the "execute" events of MembershipGroup.schedule timers that come due (pos 0xFFFFFFFF,
 * src CC_EVSRC_TIMER) to d_events; *d_events->count is written.  cc_advance_time fails with CC_ERR_UNSUPPORTED
 * when such an event is due and has no stream. */
int  cc_advance_time_events(cc_engine* e, uint64_t now, const cc_events* d_events);
/* The same with a host event stream. */
int  cc_advance_time_events_host(cc_engine* e, uint64_t now, const cc_events* h_events);

/* ---- session close / expire fan-out (ResourceManager.close :250-264, expire :238-247) -------------------
 * For each client session of h_clients, in order: every instance it owns, in java.util.HashMap iteration order of
 * ResourceManager.sessions, is closed on its state machine (LeaderElectionState.close :35-52 hands leadership to the
 * first listener, MembershipGroupState.close :36-42 publishes "leave", an AtomicValue listener is dropped; locks and
 * maps have no close handler) and leaves the dispatch table: later commits on it get CC_ST_UNKNOWN_SESSION.  Events
 * go to d_events (src CC_EVSRC_CLOSE, pos 0xFFFFFFFF) in fan-out order; *count is written.  A close that throws
 * (an election leader already cleaned by delete) ends that client's fan-out there, as the reference's loop does
 * (ResourceManager.close runs once per session; the remaining clients are closed): *h_closed = the instances closed.
 * Synchronous (control plane).                                              */
int  cc_sessions_close(cc_engine* e, const uint64_t* h_clients, uint64_t count, const cc_events* d_events, void* stream,
                       uint64_t* h_closed);
/* The expired set of cc_expire_sweep (bit s = client session id s, u64 words in HBM), closed in ascending id order. */
int  cc_sessions_expire(cc_engine* e, const uint64_t* d_bitmap, uint64_t sessions, const cc_events* d_events, void* stream,
                        uint64_t* h_closed);
/* Host-memory forms (see "host-memory entry points" above): events to a host cc_events (NULL: none may publish). */
int  cc_sessions_close_host(cc_engine* e, const uint64_t* h_clients, uint64_t count, const cc_events* h_events,
                            uint64_t* h_closed);
int  cc_sessions_expire_host(cc_engine* e, const uint64_t* h_bitmap, uint64_t sessions, const cc_events* h_events,
                             uint64_t* h_closed);

/* ---- per-kernel timing (HIP events recorded on the launch stream around every engine kernel) ----------
 * kernel ids: 0 k_part_tile, 1 k_apply_value, 2 k_unpermute, 3 k_apply_map, 4 k_map_hot (hot-key lists +
 * scan, apply_map_hot.hip), 5 k_apply_coord (coordination + value events), 6 k_events (event scan+scatter),
 * 7 k_topic_fanout (TopicState.publish and MessageBusState register / unregister / leave expansion, topic_fanout.hip;
 * launched only on engines that hold a topic or a bus). */
#define CC_PROFILE_KERNELS 8
int  cc_profile_enable(cc_engine* e, int on);
int  cc_profile_reset(cc_engine* e);
/* Accumulated device time (ms) and launch count of one kernel since the last reset (synchronizes). */
int  cc_profile_read(cc_engine* e, int kernel, double* total_ms, uint64_t* launches, const char** name);

/* Diagnostics build only (-DCC_PHASE_TIMING; scripts/probes/phase_timing.py): per-phase s_memrealtime ticks
 * (10 ns) summed over the workgroups of kernel `kernel` (0 k_part_tile, 1 k_apply_value, 2 k_unpermute) since
 * the last read, CC_PHASES entries; CC_ERR_UNSUPPORTED in the product build. */
#define CC_PHASES 8
int cc_debug_phases(cc_engine* e, int kernel, uint64_t* ticks);

/* ---- leader quorum commit index (Copycat leader [not vendored]) ------------------------
 * Per group g: N = the quorum-th largest of d_match[r*groups + g], r < replicas (r = 0 is the leader's
 * last log index), quorum = replicas/2 + 1; new = (N >= d_term_start[g] && N > d_commit_in[g]) ? N : d_commit_in[g]. */
int  cc_quorum_commit(const uint64_t* d_match, uint32_t replicas, uint64_t groups, const uint64_t* d_term_start,
                      const uint64_t* d_commit_in, uint64_t* d_commit_out, void* stream);

/* ---- session / lease expiry sweep (Copycat sessions [not vendored]) ---------------------
 * Session s is expired iff now - d_last[s] > timeout (signed difference; a keep-alive in the future never
 * expires).  Bit s of d_bitmap (u64 words, LSB first) is set for expired sessions; *d_count (u64) += expired. */
int  cc_expire_sweep(const uint64_t* d_last, uint64_t sessions, uint64_t now, uint64_t timeout,
                     uint64_t* d_bitmap, uint64_t* d_count, void* stream);

/* ---- plain device memory: for cc_quorum_commit / cc_expire_sweep and hosts that keep columns resident in HBM --------
 * (hipMalloc / hipFree / hipMemcpy on the engine's HIP runtime; cc_memcpy and cc_memset synchronize `stream`) */
#define CC_MEMCPY_H2D 1
#define CC_MEMCPY_D2H 2
#define CC_MEMCPY_D2D 3
int  cc_device_alloc(int device, uint64_t bytes, void** d_out);
int  cc_device_free(void* d_ptr);
int  cc_memcpy(void* dst, const void* src, uint64_t bytes, int kind, void* stream);
int  cc_memset(void* d_ptr, int byte, uint64_t bytes, void* stream);

/* ---- Catalyst wire format -> columns (copycat_amd/csrc/wire.cpp) ----------------------
 * A committed resource entry is InstanceCommand / InstanceQuery (@SerializeWith 30 / 31): writeLong(instance id),
 * then serializer.writeObject(operation) (InstanceOperation.java:60-69); the operation's @SerializeWith id is the
 * CC_OP_* code and its fields follow its writeObject chain (wire.cpp kSchema cites each).  Manager entries
 * (GetResource 35, CreateResource 36, DeleteResource 37, ResourceExists 38) decode to control rows.
 * Catalyst (Serializer / Buffer) is not vendored: the identifier byte before a registered type id (0 null,
 * 1..4 an id of 1..4 bytes, 5 a class name), the ids of Long / Integer / Boolean / String, byte order and the
 * UTF-8 framing are cc_wire_codec fields; the defaults below are this engine's restatement of Catalyst 1.x
 * (parity unpinned: set them from the deployment's serializer registry). */
#define CC_WIRE_ID_BOOLEAN 129
#define CC_WIRE_ID_INTEGER 132
#define CC_WIRE_ID_LONG    133
#define CC_WIRE_ID_STRING  136
typedef struct cc_wire_codec {
  uint8_t  big_endian;          /* Catalyst Buffer byte order (1: big-endian, Java's)                        */
  uint8_t  utf8_presence_byte;  /* writeUTF8 writes a boolean "not null" byte before the length               */
  uint8_t  utf8_len_bytes;      /* width of writeUTF8's length prefix                                        */
  uint8_t  reserved8;
  int32_t  id_bool, id_int, id_long, id_string;  /* registered serializer ids                                  */
  uint64_t reserved[4];
} cc_wire_codec;
void cc_wire_codec_default(cc_wire_codec* c);
/* String values and resource keys become CC_TAG_HANDLE handles through an interner (equal bytes, equal handle:
 * Java String.equals); handles are first_handle, first_handle + 1, ... in order of first appearance. */
typedef struct cc_wire_interner cc_wire_interner;
int  cc_wire_interner_create(uint64_t first_handle, cc_wire_interner** out);
int  cc_wire_interner_destroy(cc_wire_interner* in);
int  cc_wire_intern(cc_wire_interner* in, const uint8_t* bytes, uint64_t len, uint64_t* handle);
int  cc_wire_lookup(cc_wire_interner* in, uint64_t handle, uint8_t* buf, uint64_t cap, uint64_t* len);
/* java.lang.String.hashCode of an interned String (its UTF-8 bytes decoded to UTF-16 code units). */
int  cc_wire_string_hash(cc_wire_interner* in, uint64_t handle, int32_t* hash);
/* decoded rows (host memory, n each).  kind 0: a resource operation (inst = the instance slot of the instance
 * id through the engine's session registry, max_instances when unknown -> CC_ST_UNKNOWN_SESSION when applied;
 * iid = the instance id itself; op/flags/key/a/b/aux as cc_batch).  With e == NULL (no engine: host-only
 * decoding) inst is not written and iid is required.  kind 35/36/38: get/create/exists with key = the key's handle, a = the
 * CC_RES_* of the state machine class (CC_RES_NONE when not one this engine runs); kind 37: delete, b = the
 * resource id.  index and time are the log entry's own (the caller's) and are not touched. */
typedef struct cc_wire_out {
  uint32_t* inst;   /* needs an engine */
  uint64_t* iid;    /* optional with an engine */
  uint8_t*  op;
  uint8_t*  flags;
  uint64_t* key;
  uint64_t* a;
  uint64_t* b;
  uint64_t* aux;
  uint8_t*  kind;
} cc_wire_out;
/* Entry i is buf[offsets[i], offsets[i+1]) of the buf_len-byte buffer (an entry that ends past buf_len fails with its
 * row; ABI 3 added buf_len).  Fails (CC_ERR_INVALID, *bad_row = the entry) on a truncated or
 * over-long entry, an unknown operation, a null key, or a value that is neither null, Long, Integer, Boolean
 * nor String (user objects have no canonical tag); rows before *bad_row are decoded. */
int  cc_wire_decode(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in, const uint8_t* buf, uint64_t buf_len,
                    const uint64_t* offsets, uint64_t n, const cc_wire_out* out, uint64_t* bad_row);

/* ---- a batch applied up to the first commit the engine cannot hold (ABI 5; copycat_amd/csrc/host_path.hip) ----
 * Java's coordination collections are unbounded; the engine's hold cc_config.coord_cap entries.  Like
 * cc_apply_batch_host_events (h_events may be NULL), but a row that would add an entry to a full lock queue / listener
 * list / member set / queue is not applied: the call returns CC_ERR_CAPACITY with *h_applied = that row, the engine
 * state is exactly the state after rows [0, *h_applied), the events of those rows are in h_events, and rows from
 * *h_applied on are not applied (their result rows keep what the caller put there).  The host resumes at that row
 * (on an engine with a larger coord_cap or map_capacity restored from a snapshot, cc_snapshot_restore_grow above, or
 * treating the commit as failed).  On success
 * *h_applied = n.  Round 6: the same holds for a row whose map / set / multimap entry a full table region cannot
 * hold, and for a row whose events do not fit h_events' capacity (or max_events): the engine takes a device
 * checkpoint before each part of the batch and, when a part fails on one of those capacities, restores it and
 * applies the longest prefix that fits (bisection), so *h_applied is exactly that row and the state, results and
 * events are those after the rows before it.  A host with a full event stream drains it and resumes at that row. */
int  cc_apply_batch_host_prefix(cc_engine* e, const cc_batch* h_cols, uint64_t n, const cc_results* h_out,
                                const cc_events* h_events, uint64_t* h_applied);

/* ---- the same contract on device-resident columns (ABI 6; copycat_amd/csrc/host_path.hip, prefix_scan.hip) ----
 * cc_apply_batch with the stop-before-row contract of cc_apply_batch_host_prefix.  d_cols, d_out and d_events (may be
 * NULL) hold device pointers, d_events->count included, under cc_apply_batch's argument and alignment rules;
 * h_applied is a host pointer.  The call is synchronous: on return the stream is drained and the results are final.
 *   success: CC_OK, *h_applied = n; results, events, state and applied index are those of one cc_apply_batch.
 *   a full coordination collection, map table region or event stream (d_events->capacity or max_events):
 *     CC_ERR_CAPACITY with *h_applied = r < n; the state is exactly the one after rows [0, r), d_out rows [0, r) are
 *     written, rows [r, n) keep byte for byte what the caller had there, and *d_events->count = the events of rows
 *     [0, r), all present, pos relative to the batch, in publish order.
 *   any other failure is returned as it is.  n == 0: CC_OK, *h_applied = 0 (and *d_events->count = 0).  A NULL
 *   h_applied fails with CC_ERR_INVALID before anything runs; a checkpoint buffer that cannot be allocated fails the
 *   call before any row is applied.
 * The rows that may overflow a coordination collection are found on the device (no column is copied to the host);
 * on an engine with no coordination resources, no maps and no event stream the call is cc_apply_batch + cc_sync. */
int  cc_apply_batch_prefix(cc_engine* e, const cc_batch* d_cols, uint64_t n, const cc_results* d_out,
                           const cc_events* d_events, void* stream, uint64_t* h_applied);

/* ---- one global log, many engines (ABI 5; copycat_amd/csrc/split.cpp) -----------------------------
 * The reference multiplexes every resource in one Raft log (ResourceManager.java:37-39,56-72); with one engine per
 * GPU the host splits each committed batch by the rank that owns the row's resource, and merges the per-rank results
 * back into log order.  Host memory only: no engine and no GPU is involved.
 *
 * cc_split_batch: stable split of rows [0, n) of `in` (host columns; inst is required, any other column may be NULL
 * and then stays NULL).  rank_of_inst[s] (s < n_inst) is the rank owning instance slot s; a row whose inst >= n_inst
 * goes to rank 0 (whose engine answers UNKNOWN_SESSION).  counts[r] = rows of rank r.  With outs == NULL only the
 * counts are computed.  Otherwise outs[r] receives rank r's rows in log order: every column present in `in` must be
 * non-NULL in outs[r], with room for out_cap[r] rows; if counts[r] > out_cap[r] for any r the call returns
 * CC_ERR_CAPACITY with `counts` filled and nothing written.  rows (optional, world pointers, each optional) receives
 * each output row's row in `in`.  threads: worker threads (0 = hardware concurrency). */
typedef struct cc_batch_out {
  uint64_t* index;
  uint64_t* time;
  uint32_t* inst;
  uint8_t*  op;
  uint8_t*  flags;
  uint64_t* key;
  uint64_t* a;
  uint64_t* b;
  uint64_t* aux;
} cc_batch_out;
int  cc_split_batch(const cc_batch* in, uint64_t n, const uint8_t* rank_of_inst, uint32_t n_inst, uint32_t world,
                    uint32_t threads, const cc_batch_out* outs, const uint64_t* out_cap, uint64_t* counts,
                    uint64_t* const* rows);
/* cc_merge_results: the inverse for the result columns.  Row i of `out` (n rows) takes the next unread row of
 * parts[rank_of(inst[i])] (the same inst column and table the split used). */
int  cc_merge_results(const uint32_t* inst, uint64_t n, const uint8_t* rank_of_inst, uint32_t n_inst, uint32_t world,
                      uint32_t threads, const cc_results* parts, const cc_results* out);

/* ---- the same split and merge on the device: columns in HBM in, per-rank columns in HBM out (split_gpu.hip) --------
 * These calls exist from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added).
 * For a host whose columns are already in device memory (cc_wire_decode_to_device, cc_unpack_to_device, an upload):
 * cc_split_batch_device / cc_merge_results_device are cc_split_batch / cc_merge_results item by item, byte for byte,
 * with these differences:
 *   - d_in, outs[r], parts[r], d_out and d_rows are host structs / host arrays as above, whose members are device
 *     pointers, as are d_rank_of_inst and d_inst.  counts and out_cap are host memory.
 *   - No engine is involved (as cc_quorum_commit); the calls run on the device that owns `stream` (the current
 *     device for the null stream).  There is no `threads`.
 *   - d_work: caller-owned device scratch (16-byte aligned; cc_device_alloc, a torch tensor) of at least
 *     cc_split_device_bound(n, world) bytes; a smaller work_bytes is CC_ERR_INVALID.  The bound is host arithmetic:
 *     no HIP call, usable on a machine without a GPU.
 *   - Every input column that is present must be 16-byte aligned (CC_ERR_INVALID otherwise); outputs need only their
 *     natural alignment.  Inputs, outputs and the workspace must not overlap.
 *   - Every argument check that does not need the counts runs before the first HIP call.
 * Unchanged: world in [1, 256]; inst is required, any other input column may be NULL and its outputs are then left
 * alone; inst >= n_inst goes to rank 0 (n_inst == 0 with a NULL table: everything does); a rank's output columns may
 * be NULL when its count is 0; outs == NULL computes the counts only; counts[r] > out_cap[r] is CC_ERR_CAPACITY with
 * `counts` filled and nothing written to any output; an owner byte >= world is CC_ERR_INVALID with nothing written;
 * d_rows (optional, world device pointers, each optional) receives each output row's source row as u64.
 * Synchronisation: the call waits on the host exactly once, after the count and the scan kernels, for `world` counts
 * and one error word.  On CC_OK the scatter (the merge: the gather) is enqueued on `stream` and NOT waited for: the
 * outputs are ordered on `stream`, as after cc_apply_batch, and the inputs and d_work must stay untouched until the
 * stream has passed them.  A counts-only call waits and enqueues nothing.
 * Peer memory: an output pointer may be any memory the device can store to, the peer-mapped HBM of another GPU
 * included (a split straight into the owning rank's memory).  That is not exercised by the tests: the test box has
 * one GPU.  A tile is CC_SPLIT_TILE_ROWS consecutive rows (one workgroup; public so that tests can straddle it). */
#define CC_SPLIT_TILE_ROWS 4096
int  cc_split_device_bound(uint64_t n, uint32_t world, uint64_t* work_bytes);
int  cc_split_batch_device(const cc_batch* d_in, uint64_t n, const uint8_t* d_rank_of_inst, uint32_t n_inst,
                           uint32_t world, const cc_batch_out* outs, const uint64_t* out_cap, uint64_t* counts,
                           uint64_t* const* d_rows, void* d_work, uint64_t work_bytes, void* stream);
int  cc_merge_results_device(const uint32_t* d_inst, uint64_t n, const uint8_t* d_rank_of_inst, uint32_t n_inst,
                             uint32_t world, const cc_results* parts, const cc_results* d_out, void* d_work,
                             uint64_t work_bytes, void* stream);
/* Measurement aid (scripts/split_rate.py), per calling thread, off by default.  With ms != NULL: ms[0..2] = the device
 * times in milliseconds of the count kernel, the scan kernel and the scatter (or gather) kernel of this thread's last
 * device split / merge call made while enabled (0 for a kernel the call did not launch), from events recorded around
 * the launches; waits for that call's last kernel.  Then timing is switched on (enable != 0) or off for the calls that
 * follow.  Enabled calls record five events on `stream`; nothing else about them changes. */
int  cc_split_device_timing(int enable, float* ms);

/* ---- the per-rank event streams back into log order (copycat_amd/csrc/evmerge.cpp, evmerge_gpu.hip) -----------------
 * These calls exist from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added).
 * Each rank's engine publishes its events with `pos` = a row of that rank's share.  cc_merge_events turns the `world`
 * streams into the one log-ordered stream a single engine applying the whole log would have published (for a log that
 * arms no timers: a rank's timers fire on its own rows' log time).  Host memory only, no engine.
 * Inputs:
 *   - parts[r]: rank r's event stream as an engine leaves it after cc_apply_batch* on its share (host columns, host
 *     count).  A NULL count pointer means no events; a part's columns may be NULL when its count is 0.
 *   - rows[r][p]: the log row of rank r's row p: the `rows` output of cc_split_batch, strictly increasing, every value
 *     < n, no value shared by two ranks.  rows[r] may be NULL when part r has no events.
 *   - row_counts[r]: the split's counts[r] (rows of rank r); n: rows of the log.
 * Output:
 *   - `out` holds all events ordered by log row; the events of one row keep the order their rank published them in.
 *   - out->pos is the log row; target, code, src, tag and payload are copied.
 *   - *out->count (when count is non-NULL) and *total take the number of events.  Rows of `out` past the total are
 *     not touched.
 *   - A log row belongs to exactly one rank, so there are no ties across ranks: the result is fully determined by the
 *     inputs (and so is the failure reported when several events break a precondition: the lowest rank's first).
 * Preconditions, checked; a failure returns CC_ERR_INVALID, cc_last_error names the rank and the event, and nothing is
 * written to `out` (all validation completes before the first store):
 *   - A part's pos is non-decreasing.  Every batch apply produces this: commit events are appended in batch-row order
 *     (events.hip compacts the rows' event slots by an exclusive scan over the rows), a fan-out (topic publish, bus
 *     broadcast, group member list) writes its run at its publishing row's place in that scan, and a timer that fires
 *     during a batch publishes at the row whose log time fired it.
 *   - Every pos < row_counts[r].  The streams of cc_sessions_close / cc_sessions_expire / cc_advance_time_events carry
 *     pos = 0xFFFFFFFF: they are not batch events, belong to no log row, and are refused by this check.
 *   - Every rows[r][pos] < n (the index is checked before it addresses `rows`, the value before it addresses anything).
 *   - world in [1, 256]; n < 2^32; row_counts[r] <= n; every part's count, and the total, < 2^32.
 *   - Two runs of events that map to the same log row (a `rows` that is not the split's) are refused where they are
 *     seen: always by the host call, by the device call whenever the per-row runs do not add up to the events.  Neither
 *     form reads or writes out of bounds on such input.
 * Capacity; either case returns CC_ERR_CAPACITY with *total = the sum of the parts' counts and nothing written:
 *   - a part whose count exceeds its own capacity (that rank's apply had overflowed); this is checked first;
 *   - total > out->capacity; this is checked last, after the preconditions.
 * n == 0: CC_OK with *total = 0, the parts are not read (the host call stores *out->count = 0, the device call makes no
 * HIP call and stores nothing).  threads: worker threads (0 = hardware concurrency).
 *
 * cc_merge_events_device is the same call for streams in HBM, byte for byte:
 *   - parts[r] and d_out are host structs whose column pointers AND count point to device memory, as an engine takes
 *     them; d_rows is a host array of device pointers (cc_split_batch_device's d_rows); row_counts and total are host
 *     memory.  The parts' counts are read on the device.
 *   - No engine is involved; the call runs on the device that owns `stream` (the current device for the null stream).
 *   - d_work: caller-owned device scratch, 16-byte aligned, of at least cc_merge_events_device_bound(n, world) bytes
 *     (host arithmetic, no HIP call).  A smaller work_bytes, a NULL workspace, a NULL parts / d_rows / row_counts /
 *     d_out / total, or a column that lacks its natural alignment (pos, target: 4; payload, count, d_rows[r]: 8) is
 *     CC_ERR_INVALID before the first HIP call.  When every part's count pointer is NULL the call returns CC_OK with
 *     *total = 0 before the first HIP call, too.
 *   - It waits on the host exactly once, for the `world` counts, the total and the error word.  On CC_OK the gather is
 *     enqueued on `stream` and NOT waited for (with total == 0: only the store of *d_out->count); the inputs and d_work
 *     must stay untouched until the stream has passed them.  On any error nothing has been written to d_out.
 *   - Inputs, outputs and the workspace must not overlap.
 *   - Peer memory: d_out's columns may be any memory the device can store to, another GPU's peer-mapped HBM included.
 *     That is not exercised by the tests: the test box has one GPU.
 * A tile is CC_EVMERGE_TILE_ROWS consecutive log rows (one workgroup of the gather), whose events are moved
 * CC_EVMERGE_WINDOW_EVENTS at a time; both are public so that tests can straddle them. */
#define CC_EVMERGE_TILE_ROWS 4096
#define CC_EVMERGE_WINDOW_EVENTS 1024
int  cc_merge_events(const cc_events* parts, const uint64_t* const* rows, const uint64_t* row_counts, uint64_t n,
                     uint32_t world, uint32_t threads, const cc_events* out, uint64_t* total);
int  cc_merge_events_device_bound(uint64_t n, uint32_t world, uint64_t* work_bytes);
int  cc_merge_events_device(const cc_events* parts, uint64_t* const* d_rows, const uint64_t* row_counts, uint64_t n,
                            uint32_t world, const cc_events* d_out, uint64_t* total, void* d_work, uint64_t work_bytes,
                            void* stream);
/* Measurement aid (scripts/evmerge_rate.py), per calling thread, off by default, as cc_split_device_timing: ms[0..3] =
 * the device times in milliseconds of the workspace clear, the mark kernel, the two scan kernels and the gather of
 * this thread's last cc_merge_events_device call made while enabled (0 for a step the call did not reach). */
int  cc_merge_events_device_timing(int enable, float* ms);

/* ---- an event stream to its client sessions (copycat_amd/csrc/route.cpp, route_gpu.hip) ------------------------------
 * These calls exist from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added).
 * An event row names its receiver as an instance slot (`target`); the reference publishes it to the client session that
 * owns that instance (ManagedResourceSession.publish, ManagedResourceSession.java:64-71), and Copycat ships every
 * client session its own ordered list of events.  cc_route_events is a stable grouping of a stream by owning client
 * session: each session's events as one contiguous run, in the order the reference would have published them.  Host
 * memory only, no engine; cc_route_events_device is the same call for a stream in HBM, byte for byte.
 * Inputs:
 *   - `in`: the stream's columns; n_events is a host number (after cc_merge_events* it is *total; after an apply the
 *     host reads the 8-byte count).  in->count and in->capacity are not read.
 *   - session_of_inst[slot]: the host's dense ordinal, in [0, n_sessions), of the client session that owns the instance
 *     slot; id_of_inst[slot]: ManagedResourceSession.id() (both are what the host gave cc_instance_open or got from
 *     cc_get_resource); n_inst entries each.  id_of_inst and out_instance are either both NULL or both set.
 * Outputs:
 *   - `out` holds the same rows ordered by session_of_inst[target] ascending; within a session the rows keep their
 *     input order (log row first, then the state machine's publish order).  All six columns are copied unchanged: pos
 *     is data here, never an index, so result rows (CC_EVSRC_RESULT) and close / timer rows (pos 0xFFFFFFFF) are
 *     routed like every other row.  *out->count = n_events (when count is non-NULL); rows past n_events are not touched.
 *   - out_instance[j] = id_of_inst[out->target[j]].
 *   - `dir` lists only the sessions that received rows, ascending: dir->session[k] is the k-th such ordinal and
 *     dir->start[k] the first row of its run; dir->start[*dir->count] = n_events.  *dir->count and *n_active take their
 *     number.  Entries past these are not touched.  No array, neither an output nor the workspace, is sized by
 *     n_sessions: a host whose closed slots should keep their rows maps them to a dead-letter ordinal of its own.
 * Refusals: CC_ERR_INVALID with nothing written to out, out_instance or dir (all validation completes before the first
 * store), for a target >= n_inst; a table entry >= n_sessions; n_sessions == 0 with n_events > 0; n_events >= 2^32; a
 * NULL in / session_of_inst / out / dir / dir->start / dir->count / n_active, a NULL dir->session with capacity > 0, a
 * NULL column with n_events > 0, one of id_of_inst / out_instance without the other; a column that lacks its natural
 * alignment (4 bytes: pos, target, session_of_inst, dir->session, dir->start; 8 bytes: payload, count, id_of_inst,
 * out_instance).  For a bad target or table entry cc_last_error names the lowest offending event, whatever order the
 * checks ran in (the device keeps it with one atomicMin).
 * Capacity, CC_ERR_CAPACITY with nothing written: out->capacity < n_events is answered before any work (*n_active is
 * not written); dir->capacity < the number of active sessions is answered after the grouping, with *n_active set.
 * *n_active is written by CC_OK and by the directory's CC_ERR_CAPACITY only.
 * n_events == 0: CC_OK with *n_active = 0 once the arguments have passed; nothing else is stored (the device call makes
 * no HIP call).  threads: worker threads (0 = hardware concurrency).
 *
 * cc_route_events_device:
 *   - Every pointer inside d_in, d_out and d_dir, and d_session_of_inst, d_id_of_inst, d_out_instance are device
 *     pointers; the structs themselves and n_active are host memory.  No engine is involved; the call runs on the
 *     device that owns `stream` (the current device for the null stream).
 *   - d_work: caller-owned device scratch, 16-byte aligned, of at least cc_route_events_device_bound(n_events,
 *     n_sessions) bytes (host arithmetic, no HIP call: 16 B per event for the two (key, permutation) buffers and
 *     about 0.26 B per event of tile counters).  A NULL, misaligned or smaller workspace is CC_ERR_INVALID.  Every
 *     argument error above is answered before the first HIP call.
 *   - A stable least-significant-digit radix ordering of (session ordinal, event number) is built in the workspace,
 *     CC_ROUTE_DIGIT_BITS bits per round, ceil(bits(n_sessions - 1) / CC_ROUTE_DIGIT_BITS) rounds (none for one
 *     session), a workgroup per CC_ROUTE_TILE_EVENTS events; then the directory is compacted and one gather moves the
 *     rows.  Both constants are public so that tests can straddle them.
 *   - The call waits on the host exactly once, at the end, for the error word and the number of active sessions.  The
 *     kernels that store to d_out / d_out_instance / d_dir read the error word and the directory capacity on the
 *     device and store nothing when either refuses the call.  On return every output is complete.
 *   - Inputs, outputs and the workspace must not overlap.
 *   - Peer memory: the outputs may be any memory the device can store to, another GPU's peer-mapped HBM included.
 *     That is not exercised by the tests: the test box has one GPU.
 * Not covered: packing the routed stream (cc_evpack_* is specified for streams whose pos is non-decreasing; pack before
 * routing, or ship the routed columns wide), and an engine-owned copy of the two tables (the host owns the session
 * ordinals). */
#define CC_ROUTE_DIGIT_BITS 8
#define CC_ROUTE_TILE_EVENTS 4096
typedef struct cc_route_dir {   /* the sessions that received something, ascending by session ordinal */
  uint32_t* session;            /* [capacity]      session ordinal                                     */
  uint32_t* start;              /* [capacity + 1]  first row of that session's run in the routed stream;
                                                   start[*count] = n_events                            */
  uint64_t  capacity;
  uint64_t* count;              /* number of sessions with at least one row */
} cc_route_dir;
int  cc_route_events(const cc_events* in, uint64_t n_events, const uint32_t* session_of_inst,
                     const uint64_t* id_of_inst, uint32_t n_inst, uint32_t n_sessions, uint32_t threads,
                     const cc_events* out, uint64_t* out_instance, const cc_route_dir* dir, uint64_t* n_active);
int  cc_route_events_device_bound(uint64_t n_events, uint32_t n_sessions, uint64_t* work_bytes);
int  cc_route_events_device(const cc_events* d_in, uint64_t n_events, const uint32_t* d_session_of_inst,
                            const uint64_t* d_id_of_inst, uint32_t n_inst, uint32_t n_sessions,
                            const cc_events* d_out, uint64_t* d_out_instance, const cc_route_dir* d_dir,
                            uint64_t* n_active, void* d_work, uint64_t work_bytes, void* stream);
/* Measurement aid (scripts/route_rate.py), per calling thread, off by default, as cc_merge_events_device_timing:
 * ms[0..CC_ROUTE_TIMING_SLOTS) = the device times in milliseconds of k_route_key, of k_route_count, the scan kernels
 * and k_route_scatter summed over the rounds, of the directory kernels, and of k_route_gather, for this thread's last
 * cc_route_events_device call made while enabled. */
#define CC_ROUTE_TIMING_SLOTS 6
int  cc_route_events_device_timing(int enable, float* ms);

/* ---- the same decode on the GPU: wire bytes in, device columns out (copycat_amd/csrc/wire_plain.h, wire_gpu.hip) ----
 * These calls exist from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added).
 * A Copycat host holds the log's serialized entries, not columns.  cc_wire_decode_to_device takes the log segment
 * itself (host bytes + offsets) and leaves the decoded columns in device memory, byte for byte what cc_wire_decode
 * gives for the same input.  A gfx950 kernel (k_wire_decode; a workgroup per CC_WIRE_TILE_ROWS consecutive entries,
 * one lane per entry) decodes the PLAIN entries: InstanceCommand / InstanceQuery whose inner id is a known operation
 * and whose writeObject fields are all null / Long / Integer / Boolean under the codec.  Everything else ESCAPES to
 * the host decoder, in ascending row order, and its row is written over the device columns afterwards: entries that
 * carry a String (the interner is host state; but see "the device String dictionary" below, which resolves the
 * Strings an attached interner already holds), the manager entries 35-38 (the registry is host state), and every
 * malformed entry (the host decoder words the error).  Instance ids resolve through a device hash table (id -> slot)
 * that the call rebuilds from the session registry whenever the registry has changed since the last call.
 * Not covered, as in cc_wire_decode: MessageBus operations and the TopicState class name stay undecoded (they escape
 * and fail or decode exactly as before).  There is no device-resident byte-buffer form, no pipeline (one upload, one
 * decode), and the decoded columns are not packed. */
#define CC_WIRE_TILE_ROWS 2048
typedef struct cc_wire_control {  /* one manager entry (kind 35-38) of the segment, fields as in cc_wire_out */
  uint64_t row;
  uint64_t kind;
  uint64_t key;
  uint64_t a;
  uint64_t b;
} cc_wire_control;
typedef struct cc_wire_stats {
  uint64_t rows;         /* entries of the call */
  uint64_t device_rows;  /* decoded by k_wire_decode */
  uint64_t host_rows;    /* escaped: decoded by the host fallback */
} cc_wire_stats;
/* h_buf / h_offsets as cc_wire_decode's buf / offsets (only bytes [offsets[0], offsets[n]) are copied; neither needs
 * any alignment).  d_cols: device columns of n rows, each 16-byte aligned; inst, op, flags, key, a, b, aux are
 * required, index and time are not touched.  d_iid (optional, 16-byte aligned): the instance ids.  An escaped row
 * gets the host decoder's row; a manager entry's row therefore holds inst = max_instances, op = flags = 0 and its key /
 * a / b, and is also returned as h_ctl[k] = {row, kind, key, a, b}, ascending by row, *ctl_count of them.  More than
 * ctl_cap of them: CC_ERR_CAPACITY with *ctl_count = the number needed; the columns are valid, and calling again with
 * room is harmless (interning is idempotent).  The call is synchronous on `stream`.
 * Failure: the first failing row in row order wins, exactly as in cc_wire_decode, be it a malformed entry or an
 * offsets violation: the same return code, cc_last_error text and *bad_row.  Device rows before it are decoded, the
 * interner holds the Strings of the rows before it and no others, and no String key is registered
 * (cc_handle_hashes); on success String keys are registered as cc_wire_decode does.  stats may be NULL. */
int  cc_wire_decode_to_device(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in, const uint8_t* h_buf,
                              uint64_t buf_len, const uint64_t* h_offsets, uint64_t n, const cc_batch_out* d_cols,
                              uint64_t* d_iid, cc_wire_control* h_ctl, uint64_t ctl_cap, uint64_t* ctl_count,
                              cc_wire_stats* stats, void* stream, uint64_t* bad_row);
/* ---- the device String dictionary (opt-in, per engine; symbols added under the unchanged CC_ABI_VERSION 6) ----
 * After the first sight of a key universe nearly every String of a log is interned already, and looking those up
 * needs no host state the device cannot hold.  cc_wire_dict_attach uploads the interner's Strings as a hash table
 * plus a byte pool; from then on a decode on the device (cc_wire_decode_to_device, cc_apply_wire_host) that passes
 * the same interner also decodes entries whose Strings are all in the dictionary, byte for byte as cc_wire_decode: a
 * hit is a hit only after every byte compared equal, and the handle is first_handle + the String's rank.  What still
 * escapes: a String the interner has not seen (its handle is its first-occurrence rank, which only the host decoder,
 * going through the escaped rows in row order, can assign), a String longer than CC_WIRE_STR_MAX bytes, and a String
 * KEY whose String.hashCode is not yet registered on this engine (cc_handle_hashes): the host fallback decodes that
 * row and registers the hash as before, so the registered handles after a call are exactly cc_wire_decode's.  Every
 * decode first brings the dictionary up to date with the interner (Strings interned by cc_wire_intern or by an
 * earlier call's escapes) and with the engine's registered hashes (cc_handle_hashes, cc_snapshot_restore); the
 * upload is the new pool bytes and the changed cells, the whole table only when it doubles.  A call that passes
 * another interner (or one re-created at the same address) decodes as if nothing were attached.  The dictionary is
 * no part of a snapshot; cc_engine_destroy detaches.  The interner must outlive the attachment or be detached first.
 * CC_WIRE_STR_MAX: the decode hashes and compares a String in one lane, 8 bytes a step, so the bound caps the
 * divergent loop at 32 steps and the longest device-decoded entry at 836 bytes, a twentieth of the kernel's LDS
 * window; resource keys, member names and short messages are far below it, and a longer String is a payload whose
 * host decode is small beside its upload. */
#define CC_WIRE_STR_MAX 256
typedef struct cc_wire_dict_info {
  uint64_t strings;            /* Strings in the dictionary */
  uint64_t long_strings;       /* Strings of the interner left out: longer than CC_WIRE_STR_MAX (or past rank 2^32 - 2) */
  uint64_t pool_bytes;         /* the byte pool (every String padded to 8 bytes) */
  uint64_t cells;              /* table cells (a power of two, at least twice `strings`) */
  uint64_t full_uploads;       /* whole-table uploads so far (the attach, and every doubling) */
  uint64_t last_sync_strings;  /* Strings added by the last sync (a decode syncs when the interner or the hashes moved) */
  uint64_t last_str_rows;      /* rows of the last decode that the device decoded and that carried a resolved String */
} cc_wire_dict_info;
int  cc_wire_dict_attach(cc_engine* e, cc_wire_interner* in);
int  cc_wire_dict_detach(cc_engine* e);   /* frees it; decodes behave as before the attach.  Harmless when not attached */
int  cc_wire_dict_get_info(cc_engine* e, cc_wire_dict_info* out);  /* CC_ERR_STATE when nothing is attached */
/* The stage times of the engine's last decode on the device (either call), from HIP events: h_ms[0] the H2D of the
 * bytes and offsets, h_ms[1] k_wire_decode, h_ms[2] the escape round trip (the count, and the bitmap when any row
 * escaped, back to the host); milliseconds.  The host fallback and the patch come after and are not in it. */
int  cc_wire_timeline(cc_engine* e, float* h_ms);
/* Decode into engine-owned staging columns and apply rows [0, r) with cc_apply_batch, r = the first manager entry's
 * row, or n: *h_applied = r, and when r < n, *ctl is that entry.  The host runs the manager command and calls again
 * from row r + 1: the rows after a manager entry must see the registry it leaves behind, and only the Strings of
 * rows <= r are interned.  h_index / h_time: the entries' log indices / times (h_time may be NULL); results and
 * events return to the host as from cc_apply_batch_host_events (h_events may be NULL: then as cc_apply_batch_host),
 * under its size rules, for rows [0, r).  One upload, one decode, one apply, wide results back: a host that hands over
 * whole segments calls cc_apply_wire_host_packed (below, after the packed formats), which pipelines the same work. */
int  cc_apply_wire_host(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in, const uint8_t* h_buf,
                        uint64_t buf_len, const uint64_t* h_offsets, uint64_t n, const uint64_t* h_index,
                        const uint64_t* h_time, const cc_results* h_out, const cc_events* h_events,
                        uint64_t* h_applied, cc_wire_control* ctl);

/* ---- packed host batches (copycat_amd/csrc/pack.cpp, unpack.hip, host_path.hip) ---------------------------------------
 * The host-memory calls above ship index / key / a / b / aux as full u64 and inst as u32: 30 B per commit for the six
 * columns of a value batch, and the H2D of those bytes is most of a PCIe-inclusive step.  In a committed log a run of
 * consecutive rows has indices, instance slots and operands close to each other, so a batch packs exactly into a
 * per-block base plus narrow offsets; a gfx950 kernel (k_unpack) widens it back into the ordinary columns in HBM.
 *
 * One contiguous, 16-byte-aligned host blob per batch:  header | directory | data
 *   header     cc_pack_header (64 B)
 *   directory  cc_pack_block[blocks] (160 B each), block k = rows [4096 k, min(n, 4096 (k + 1)))
 *   data       per block one data area; per present column its packed rows at `offset` inside the area
 * Every offset is a multiple of 16; block areas lie after the directory, ascending and non-overlapping; a column's
 * packed rows (rows * width bytes, rounded up to 16) lie inside its block's area and overlap no other column's.
 * `present` bit c is column c in cc_batch order (index, time, inst, op, flags, key, a, b, aux); a column is present in
 * every block or in none (the NULL column pointer of cc_batch).  Entries of absent columns are ignored (written 0).
 *
 *   mode         value of a row                                              widths (bytes)
 *   CC_PK_FOR    base + zero_extend(offset), modulo the column's native      0, 1, 2, 4, 8, never above the native
 *                width (64 bits; inst 32; op and flags 8)                    width; 0: every row equals base; the
 *                                                                            native width is written with base 0 (raw)
 *   CC_PK_REL_A  a[row] + sign_extend(offset) modulo 2^64; column b only,    1, 2, 4
 *                and only with a present
 * Offsets are little-endian.  The encoder picks, per block and column, the narrowest exact encoding among FOR with
 * base = the unsigned minimum, FOR with base = the signed minimum (64-bit columns) and REL_A (b); ties go to FOR, then
 * to the unsigned base.  Decoding reproduces the caller's columns byte for byte, rows an op does not use included:
 * the format is exact for every input and has no escape path. */
#define CC_PACK_BLOCK_ROWS 4096
#define CC_PACK_VERSION    1
#define CC_PACK_MAGIC      1263551299  /* "CCPK" little-endian */
#define CC_PACK_COLUMNS    9
#define CC_PK_FOR          0
#define CC_PK_REL_A        1

typedef struct cc_pack_header {
  uint32_t magic;       /* CC_PACK_MAGIC */
  uint32_t version;     /* CC_PACK_VERSION */
  uint64_t n;           /* rows */
  uint64_t blocks;      /* ceil(n / CC_PACK_BLOCK_ROWS) */
  uint64_t bytes;       /* the whole blob */
  uint32_t present;     /* 9-bit column mask */
  uint32_t block_rows;  /* CC_PACK_BLOCK_ROWS */
  uint64_t reserved[3];
} cc_pack_header;

typedef struct cc_pack_col {
  uint8_t  mode;        /* CC_PK_* */
  uint8_t  width;       /* bytes per row */
  uint16_t reserved16;
  uint32_t offset;      /* of the column's packed rows inside the block's data area */
  uint64_t base;
} cc_pack_col;

typedef struct cc_pack_block {
  uint32_t rows;        /* CC_PACK_BLOCK_ROWS, or the tail's */
  uint32_t bytes;       /* length of the block's data area */
  uint64_t offset;      /* of the block's data area from the blob start */
  cc_pack_col col[9];
} cc_pack_block;

/* Host side, no GPU involved.  cc_pack_bound: the worst-case blob size of n rows with the `present` columns.
 * cc_pack_batch: h_cols (NULL column = absent) -> h_blob (16-byte aligned, cap bytes); *bytes = the blob's size; a cap
 * too small returns CC_ERR_CAPACITY with *bytes = the size needed and writes nothing (so a cap below cc_pack_bound is
 * sized first, one more min / max pass over the columns: pass the bound).  One block at a time per thread (the block
 * stays in cache between the min / max pass and the narrow write); threads = 0: hardware concurrency.
 * cc_pack_check: the single validator every consumer runs first: magic, version, sizes, the directory inside the blob,
 * every block's rows (their sum = n), every offset aligned, inside its area and non-overlapping, mode and width legal
 * for the column, REL_A only on b and only with a.  Any violation is CC_ERR_INVALID (message: cc_last_error); a blob
 * that passes decodes without a read outside `bytes` or a write outside n output rows.  *n / *present (optional).
 * cc_unpack_batch: the host decoder (h_out: every present column non-NULL, n rows). */
int  cc_pack_bound(uint64_t n, uint32_t present, uint64_t* bytes);
int  cc_pack_batch(const cc_batch* h_cols, uint64_t n, void* h_blob, uint64_t cap, uint32_t threads, uint64_t* bytes);
int  cc_pack_check(const void* h_blob, uint64_t bytes, uint64_t* n, uint32_t* present);
int  cc_unpack_batch(const void* h_blob, uint64_t bytes, const cc_batch_out* h_out, uint32_t threads);

/* Copy a packed host blob to the device and decode it into the caller's device columns (n rows each, present columns
 * non-NULL, 16-byte aligned); stream-ordered on `stream` (the blob is copied into an engine-owned buffer that the next
 * call on this engine reuses: sync before the host blob or that engine is used again).  For hosts that keep columns
 * resident (cc_apply_batch, cc_apply_batch_prefix) but receive them over PCIe.  cc_pack_check runs first: a malformed
 * blob never reaches the GPU. */
int  cc_unpack_to_device(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_batch_out* d_cols, void* stream);

/* The encoder on the device: device columns (d_cols: a host struct of device pointers, NULL column = absent, every
 * present one 16-byte aligned, n rows) -> a batch blob in the caller's host memory (h_blob 16-byte aligned), for a host
 * whose columns are already in HBM (cc_wire_decode_to_device, cc_unpack_to_device, a share of cc_split_batch_device)
 * and must leave it narrow.  The call exists from this commit on, under the unchanged CC_ABI_VERSION 6.  A gfx950
 * encoder (pack_enc.hip) builds the blob in engine-owned staging on `stream`; only header + directory + used data bytes
 * are copied.  Synchronous: on return the stream is drained and the blob is final, byte for byte cc_pack_batch's for the
 * same columns at any thread count (reserved words and absent columns' entries 0, areas back to back in block order,
 * the paddings zero), so every consumer of a batch blob takes it.  A misaligned column or blob: CC_ERR_INVALID;
 * cap < cc_pack_bound(n, present): CC_ERR_CAPACITY with *bytes = the bound, before any launch.  n == 0: a header-only
 * blob, as cc_pack_batch. */
int  cc_pack_from_device(cc_engine* e, const cc_batch* d_cols, uint64_t n, void* h_blob, uint64_t cap, uint64_t* bytes,
                         void* stream);

typedef struct cc_packed_opts {
  uint64_t chunk_rows;  /* rows per pipeline chunk; 0 = 16 Mi; rounded up to whole blocks, capped by max_batch and the
                           engine's extended sub-batch */
  uint32_t flags;       /* CC_PACKED_* */
  uint32_t reserved32;
  uint64_t reserved[2];
} cc_packed_opts;
#define CC_PACKED_TIMELINE 1  /* record HIP events around every chunk's stages (cc_packed_timeline) */
/* cc_apply_batch_host_events on a packed blob (h_events may be NULL: then as cc_apply_batch_host; opts may be NULL),
 * pipelined inside the library: the batch goes in chunks of whole blocks, and while chunk k is decoded and applied on
 * the engine's stream, chunk k+1's bytes travel H2D on a copy-in stream and chunk k-1's results travel D2H on a
 * copy-out stream, straight into h_out rows [lo, hi).  Page-lock h_blob and h_out (cc_host_register) or the copies
 * do not overlap.  Results, events (pos = batch rows), state and applied index are those of one
 * cc_apply_batch_host_events call on the decoded columns.
 * Failure: that of consecutive cc_apply_batch_host_events calls over the chunks.  The call stops at the first failing
 * chunk and returns its code; *h_rows_done (may be NULL) = the rows of the chunks fully applied (n on success);
 * *h_events->count = the events of those chunks plus the failing chunk's count; result rows of chunks not applied
 * keep what the caller had.  With an event stream or on an engine with maps each chunk runs under a device checkpoint
 * (as the parts of cc_apply_batch_host_prefix do), and a chunk that fails on a full event stream or map table region
 * is rolled back: the state is then exactly the one after *h_rows_done rows, where the host resumes.  A malformed
 * blob is CC_ERR_INVALID before anything is copied or launched.  n == 0: CC_OK, no launch, *h_events->count = 0. */
int  cc_apply_batch_host_packed(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_results* h_out,
                                const cc_events* h_events, const cc_packed_opts* opts, uint64_t* h_rows_done);

/* The stage times of the last cc_apply_batch_host_packed call made with CC_PACKED_TIMELINE, from HIP events: *chunks =
 * the chunks that completed; h_ms (4 floats per chunk, room for cap chunks) = H2D, decode, apply, D2H milliseconds. */
int  cc_packed_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms);

/* hipHostRegister / hipHostUnregister: page-lock caller memory (a packed blob, result columns, an off-heap segment) so
 * the asynchronous copies of the host calls overlap with the kernels.  NULL or zero bytes: CC_ERR_INVALID. */
int  cc_host_register(void* h_ptr, uint64_t bytes);
int  cc_host_unregister(void* h_ptr);

/* ---- packed result blobs (copycat_amd/csrc/respack.cpp, respack.hip, host_path.hip) ----------------------------------
 * The result-blob calls exist from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added).
 * The host calls above return results wide: 1 status byte + 8 value bytes per commit.  Within a block of consecutive
 * rows the values are counters close to each other and the statuses are mostly one byte value, so cc_results packs the
 * way the operands do.  A gfx950 encoder (respack.hip) writes the blob in HBM and only the narrow bytes travel D2H.
 *
 * One contiguous, 16-byte-aligned blob:  header | directory | data
 *   header     cc_pack_header (64 B): magic CC_RESPACK_MAGIC, version CC_RESPACK_VERSION, present = 3,
 *              block_rows = CC_PACK_BLOCK_ROWS
 *   directory  cc_respack_block[blocks] (48 B each), block k = rows [4096 k, min(n, 4096 (k + 1)))
 *   data       per block one data area; per column its rows at `offset` inside the area (rows * width bytes, rounded
 *              up to 16, the padding zero)
 * col[0] is status, col[1] is value.  Every offset is a multiple of 16; block areas lie after the directory, ascending
 * in block order and non-overlapping; a column's rows lie inside its block's area and overlap no other column's.
 * The only mode is CC_PK_FOR:
 *   value    base + zero_extend(offset) modulo 2^64; widths 0, 1, 2, 4, 8; width 8 is the raw column with base 0
 *   status   widths 0, 1; width 1 is the raw column with base 0; width 0: every row equals base
 * The encoder takes, per block and column, the narrowest exact width among base = the unsigned minimum and (value)
 * base = the signed minimum; a tie goes to the unsigned base.  The blob a full encode writes (cc_respack_pack,
 * cc_respack_from_device, a cc_apply_batch_host_packed_results call that applies every chunk) is a function of the
 * result columns alone: status area first, value area after it, block areas back to back from the directory's end;
 * neither the thread count nor the GPU / host split nor the chunking changes a byte.  Decoding reproduces the wide
 * columns byte for byte, the value bytes of NULL-tagged rows and the 0xFF / 0xA5 prefill of a row no kernel wrote
 * included; there is no escape path. */
#define CC_RESPACK_MAGIC   1380991811  /* "CCPR" little-endian */
#define CC_RESPACK_VERSION 1
#define CC_RESPACK_COLUMNS 2

typedef struct cc_respack_block {
  uint32_t rows;        /* CC_PACK_BLOCK_ROWS, or the tail's */
  uint32_t bytes;       /* length of the block's data area */
  uint64_t offset;      /* of the block's data area from the blob start */
  cc_pack_col col[2];   /* status, value */
} cc_respack_block;

/* Host side, no GPU involved.  cc_respack_bound: the worst-case blob size of n rows.  cc_respack_pack: the reference
 * encoder, h_results (n rows) -> h_blob (16-byte aligned, cap bytes); *bytes = the blob's size; a cap too small
 * returns CC_ERR_CAPACITY with *bytes = the size needed and writes nothing.  cc_respack_check: the single validator
 * (magic, version, present, sizes, the directory inside the blob, every block's rows and their sum, every offset
 * aligned, inside its area and non-overlapping, mode and width legal for the column); any violation is CC_ERR_INVALID
 * with a message that names the "result blob"; *n optional.  cc_respack_unpack: the host decoder (validator first;
 * h_out: n rows each). */
int  cc_respack_bound(uint64_t n, uint64_t* bytes);
int  cc_respack_pack(const cc_results* h_results, uint64_t n, void* h_blob, uint64_t cap, uint32_t threads,
                     uint64_t* bytes);
int  cc_respack_check(const void* h_blob, uint64_t bytes, uint64_t* n);
int  cc_respack_unpack(const void* h_blob, uint64_t bytes, const cc_results* h_out, uint32_t threads);

/* Encode device result columns (d_results: status and value in HBM, n rows, both 16-byte aligned) into a result blob
 * in the caller's host memory: the counterpart of cc_unpack_to_device for hosts that keep columns resident but take
 * results over PCIe.  The blob is built in engine-owned staging on `stream`; only header + directory + used data bytes
 * are copied.  Synchronous: on return the stream is drained and the blob is final, byte for byte cc_respack_pack's.
 * cap < cc_respack_bound(n): CC_ERR_CAPACITY with *bytes = the bound, before any launch.  n == 0: a header-only blob. */
int  cc_respack_from_device(cc_engine* e, const cc_results* d_results, uint64_t n, void* h_blob, uint64_t cap,
                            uint64_t* bytes, void* stream);

/* The decoder on the device (exists from this commit on, under the unchanged CC_ABI_VERSION 6): copy a result blob in
 * host memory to the device and decode it into the caller's device columns (d_out: status and value in HBM, header.n
 * rows each, 16-byte aligned), e.g. a rank's answer on its way into cc_merge_results_device.  The counterpart of
 * cc_unpack_to_device, with its staging and stream rules: stream-ordered on `stream` and not waited for; the blob is
 * copied into the engine-owned buffer cc_unpack_to_device uses, which the next such call on this engine reuses: sync
 * before the host blob or that engine is used again.  cc_respack_check runs first: a malformed blob is CC_ERR_INVALID
 * and never reaches the GPU.  The decoded columns are cc_respack_unpack's byte for byte (unpack_res.hip).  A
 * header-only blob writes nothing. */
int  cc_respack_to_device(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_results* d_out, void* stream);

/* cc_apply_batch_host_packed with the result rows replaced by a result blob: the same chunking, streams, checkpoint /
 * rollback and event-stream rules; state, events, applied index and *h_rows_done are exactly those of
 * cc_apply_batch_host_packed on the same input.  Per chunk the encoder runs on the engine's stream after the apply,
 * and the copy-out stream sends the chunk's directory entries and its data bytes, and only those, into h_res_blob.
 * On every return after argument validation h_res_blob is a valid result blob (*res_bytes its size) of rows
 * [0, header.n): the rows whose results the wide call would have copied out, i.e. the applied chunks plus a failing
 * chunk that stays applied; a rolled-back chunk is excluded (then header.n == *h_rows_done).  Decoded, it equals the
 * wide call's result rows byte for byte.  When a call stops early the directory keeps the room of all n rows' blocks,
 * so the data areas start where they do in the full blob.  h_res_blob NULL or not 16-byte aligned: CC_ERR_INVALID;
 * res_cap < cc_respack_bound(n): CC_ERR_CAPACITY with *res_bytes = the bound, before anything is copied or launched.
 * opts->flags accepts CC_PACKED_TIMELINE only.  Page-lock both blobs (cc_host_register) or the copies do not overlap. */
int  cc_apply_batch_host_packed_results(cc_engine* e, const void* h_blob, uint64_t bytes, void* h_res_blob,
                                        uint64_t res_cap, uint64_t* res_bytes, const cc_events* h_events,
                                        const cc_packed_opts* opts, uint64_t* h_rows_done);

/* The stage times of the last cc_apply_batch_host_packed_results call made with CC_PACKED_TIMELINE: *chunks = the
 * chunks that completed; h_ms (5 floats per chunk, room for cap chunks) = H2D, decode, apply, encode, D2H ms. */
int  cc_packed_results_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms);

/* ---- packed event blobs (copycat_amd/csrc/evpack.cpp, evpack.hip, host_path.hip) -------------------------------------
 * The event-blob calls exist from this commit on, under the unchanged CC_ABI_VERSION 6 (symbols are only added).
 * A cc_events row is 19 B wide (pos, target u32; code, src, tag u8; payload u64), and a fan-out (a topic publish, a
 * group join or leave) writes one row per listener: the event stream is the widest of a host's three streams.  Inside
 * a block of consecutive events pos is non-decreasing and spans few rows, code / src / tag are one value or a few,
 * target spans the instance slots of a few resources, and a fan-out's payload is one value per publishing row.  A
 * gfx950 encoder (evpack.hip) writes the blob in HBM and only the narrow bytes travel D2H.
 *
 * One contiguous, 16-byte-aligned blob:  header | directory | data
 *   header     cc_pack_header (64 B): magic CC_EVPACK_MAGIC, version CC_EVPACK_VERSION, n = events, present = 0x3F,
 *              block_rows = CC_PACK_BLOCK_ROWS
 *   directory  cc_evpack_block[blocks] (112 B each), block k = events [4096 k, min(n, 4096 (k + 1)))
 *   data       per block one data area; the six columns lie in it in cc_events order (pos, target, code, src, tag,
 *              payload), each rows * width bytes (or its table, below) rounded up to 16, the padding zero
 * Every offset is a multiple of 16; block areas lie back to back from the directory's end, in block order.
 *   CC_PK_FOR     value = base + zero_extend(offset), modulo the column's native width
 *                   pos, target     widths 0, 1, 2, 4; 4 is the raw column with base 0; base = the unsigned minimum
 *                   code, src, tag  widths 0, 1; 1 is the raw column with base 0
 *                   payload         widths 0, 1, 2, 4, 8; 8 is the raw column with base 0; the narrowest of base = the
 *                                   unsigned minimum and base = the signed minimum, a tie to the unsigned base (the
 *                                   result blob's value rule)
 *   CC_PK_BY_POS  payload only: the column is a table indexed by the row's pos offset,
 *                   payload[row] = base + zero_extend(table[pos[row] - pos.base])
 *                 cc_pack_col.reserved16 = the table's entries E, the stored bytes are r16(E * width), an entry no row
 *                 refers to is 0.  Legal only when the block's pos column has width 0, 1 or 2.  The encoder may use it
 *                 when for every row i >= 1 of the block pos[i] >= pos[i-1], and pos[i] == pos[i-1] implies
 *                 payload[i] == payload[i-1]; then E = pos_max - pos_min + 1, base and width are the FOR rule's, and
 *                 it is chosen iff width > 0 and r16(E * width) < r16(rows * width) (a tie goes to FOR).
 * A row is decodable on its own: one directory entry, one pos read and (BY_POS) one table read.  Decoding reproduces
 * the six columns byte for byte for every input; there is no escape path.  The blob of a full encode is a function of
 * the event columns alone: the host encoder at any thread count, the kernels and the pipelined call at any chunking
 * write the same bytes. */
#define CC_EVPACK_MAGIC    1162888003  /* "CCPE" little-endian */
#define CC_EVPACK_VERSION  1
#define CC_EVPACK_COLUMNS  6
#define CC_PK_BY_POS       2

typedef struct cc_evpack_block {
  uint32_t rows;        /* CC_PACK_BLOCK_ROWS, or the tail's */
  uint32_t bytes;       /* length of the block's data area */
  uint64_t offset;      /* of the block's data area from the blob start */
  cc_pack_col col[6];   /* pos, target, code, src, tag, payload */
} cc_evpack_block;

/* Host side, no GPU involved.  cc_evpack_bound: the worst-case blob size of n events.  cc_evpack_pack: the reference
 * encoder; it takes h_events' column pointers only (capacity and count are ignored), n events -> h_blob (16-byte
 * aligned, cap bytes); *bytes = the blob's size; a cap too small returns CC_ERR_CAPACITY with *bytes = the size needed
 * and writes nothing.  cc_evpack_check: the single validator (every check cc_respack_check makes, and for BY_POS:
 * payload column only, pos width <= 2, 1 <= E <= 4096, table bytes = r16(E * width), every pos offset of the block
 * < E); any violation is CC_ERR_INVALID with a message that names the "event blob"; *n optional.  A blob that passes
 * decodes with no read outside `bytes` and no write outside n rows.  cc_evpack_unpack: the host decoder (validator
 * first; h_out->capacity >= n or CC_ERR_CAPACITY; *h_out->count = n when count is non-NULL). */
int  cc_evpack_bound(uint64_t n, uint64_t* bytes);
int  cc_evpack_pack(const cc_events* h_events, uint64_t n, void* h_blob, uint64_t cap, uint32_t threads, uint64_t* bytes);
int  cc_evpack_check(const void* h_blob, uint64_t bytes, uint64_t* n);
int  cc_evpack_unpack(const void* h_blob, uint64_t bytes, const cc_events* h_out, uint32_t threads);

/* Encode a device event stream (d_events: device columns, pos / target / payload 16-byte aligned, and its device count
 * word) into an event blob in the caller's host memory, for hosts that keep columns resident (after cc_apply_batch,
 * cc_apply_batch_prefix, cc_sessions_close / cc_sessions_expire, cc_advance_time_events) but take events over PCIe.
 * The call drains `stream`, reads *d_events->count, encodes min(count, capacity) events in engine-owned staging and
 * copies only header + directory + used data bytes.  Synchronous; the blob is byte for byte cc_evpack_pack's.  *count
 * (optional) = the device count; when it exceeds capacity the call returns CC_ERR_CAPACITY after writing the first
 * `capacity` events' blob, as the wide host forms do.  cap_bytes < cc_evpack_bound(capacity): CC_ERR_CAPACITY with
 * *bytes = the bound, before any launch.  Zero events: a header-only blob. */
int  cc_evpack_from_device(cc_engine* e, const cc_events* d_events, void* h_blob, uint64_t cap_bytes, uint64_t* bytes,
                           uint64_t* count, void* stream);

/* The decoder on the device (exists from this commit on, under the unchanged CC_ABI_VERSION 6): copy an event blob in
 * host memory to the device and decode it into a device event stream (d_out: six device columns, each 16-byte aligned,
 * and the device count word), with cc_respack_to_device's staging and stream rules (stream-ordered, not waited for;
 * sync before the host blob or the engine is used again).  cc_evpack_check runs first: a malformed blob is
 * CC_ERR_INVALID and never reaches the GPU; d_out->capacity < header.n: CC_ERR_CAPACITY, nothing copied or launched.
 * The decoded columns are cc_evpack_unpack's byte for byte, a CC_PK_BY_POS payload included (unpack_res.hip), and the
 * DEVICE word *d_out->count is set to header.n on the stream: d_out is then an event stream cc_merge_events_device
 * and cc_evpack_from_device take as it stands.  A header-only blob writes no column and sets the count to 0. */
int  cc_evpack_to_device(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_events* d_out, void* stream);

/* cc_apply_batch_host_packed_results with the host event stream replaced by an event blob of at most ev_capacity
 * events.  State, result blob, applied index, *h_rows_done and the return code are exactly those of that call made with
 * a wide host event stream of capacity = ev_capacity; *ev_count is what it leaves in *h_events->count.  Every chunk's
 * events are appended to engine-owned device columns after those of the chunks before, pos is shifted to batch rows on
 * the device, and no wide event byte crosses PCIe.  On every return after argument validation h_ev_blob is a valid
 * event blob (*ev_bytes its size) of the events of rows [0, *h_rows_done), the chunks fully applied; a failing or
 * rolled-back chunk's events are not in it.  Decoded, it equals the first header.n rows of the wide call's event
 * columns byte for byte, and its bytes do not depend on the chunking.  The blob is encoded once, after the last chunk,
 * and leaves in one D2H: the directory's length, and with it every data offset, is known only with the last chunk's
 * count.  h_ev_blob NULL or not 16-byte aligned, ev_bytes or ev_count NULL: CC_ERR_INVALID; ev_cap_bytes <
 * cc_evpack_bound(ev_capacity): CC_ERR_CAPACITY with *ev_bytes = the bound, before anything is copied or launched. */
int  cc_apply_batch_host_packed_events(cc_engine* e, const void* h_blob, uint64_t bytes, void* h_res_blob,
                                       uint64_t res_cap, uint64_t* res_bytes, void* h_ev_blob, uint64_t ev_capacity,
                                       uint64_t ev_cap_bytes, uint64_t* ev_bytes, uint64_t* ev_count,
                                       const cc_packed_opts* opts, uint64_t* h_rows_done);

/* The stage times of the last cc_apply_batch_host_packed_events call made with CC_PACKED_TIMELINE: *chunks = the
 * chunks that completed; h_ms (7 floats per chunk, room for cap chunks) = H2D, decode, apply, result encode, result
 * D2H, event encode, event D2H milliseconds.  The event blob is encoded and sent once per call: the last two figures
 * are the call's, repeated in every chunk's row. */
int  cc_packed_events_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms);

/* ---- the log segment through the pipeline: wire bytes in, packed results and events out (host_path.hip, wire_gpu.hip) --
 * cc_apply_wire_host, cut into the chunks of the packed pipeline: while chunk k is decoded (k_wire_decode) and applied,
 * chunk k + 1's entry bytes, offsets and its piece of the aux blob travel H2D, and chunk k - 1's encoded results travel
 * D2H.  The wire does not carry index and time: they arrive as a cc_pack_batch blob of n rows whose present columns are
 * index, or index | time (cc_pack_check runs first; another row count, no index, or any other column: CC_ERR_INVALID
 * before anything is copied).  Results leave as a packed result blob, events as a packed event blob (h_ev_blob NULL: no
 * event stream, a publishing op fails its chunk as in cc_apply_batch_host); the blob arguments follow
 * cc_apply_batch_host_packed_events, bounds and checks included.  opts: chunk_rows and CC_PACKED_TIMELINE.
 *
 * Chunks are whole CC_PACK_BLOCK_ROWS blocks (a block is two CC_WIRE_TILE_ROWS tiles), at most chunk_rows rows, and
 * shortened, block by block but never below one block, until a chunk's entry bytes are at most 1 GiB (the staging cap).
 * With the segment cut that way, state, results (cc_respack_unpack), events (cc_evpack_unpack, pos = segment rows), the
 * applied index, the interner, the registered String.hashCodes, *ctl and the error are what consecutive
 * cc_apply_wire_host calls over those chunks produce; rows are reported as segment rows (ctl->row, *bad_row and the
 * "wire row N" of cc_last_error).  Neither blob's bytes depend on chunk_rows.
 *   manager entry at row r   CC_OK, *h_rows_done = r, *ctl = the entry; rows [0, r) are applied and in the blobs;
 *                            nothing of a later row is applied, interned or registered.  Call again from row r + 1.
 *   an entry that fails to decode, or an offsets violation (offsets decrease, an entry ends past buf_len)
 *                            its chunk is not applied: the error of cc_wire_decode_to_device, *bad_row = the row,
 *                            *h_rows_done = the rows of the chunks before, both blobs valid for exactly those rows.
 *                            The host checks only a chunk's two end offsets before its copy; the offsets between them
 *                            are checked on the device, so no byte outside [buf, buf + buf_len) is ever read.
 *   full event stream or map table region
 *                            CC_ERR_CAPACITY, the chunk rolled back, as cc_apply_batch_host_packed_events.
 *   n == 0                   CC_OK, header-only blobs, nothing launched.
 * When *h_rows_done < n and the call returned CC_OK, *ctl is the manager entry; otherwise *ctl is not written.  Every
 * stream is drained before the call returns.  Page-lock buf, offsets and the blobs or the copies do not overlap. */
typedef struct cc_wire_segment {
  const uint8_t*  buf;       uint64_t buf_len;   /* entry bytes, no alignment needed            */
  const uint64_t* offsets;   uint64_t n;         /* n + 1 offsets into buf                      */
  const void*     aux_blob;  uint64_t aux_bytes; /* cc_pack_batch blob of n rows, present =     */
                                                 /* index, or index | time; 16-byte aligned     */
} cc_wire_segment;
int  cc_apply_wire_host_packed(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in,
                               const cc_wire_segment* seg, void* h_res_blob, uint64_t res_cap, uint64_t* res_bytes,
                               void* h_ev_blob, uint64_t ev_capacity, uint64_t ev_cap_bytes, uint64_t* ev_bytes,
                               uint64_t* ev_count, const cc_packed_opts* opts, uint64_t* h_rows_done,
                               cc_wire_control* ctl, uint64_t* bad_row);
/* The stage times of the last cc_apply_wire_host_packed call made with CC_PACKED_TIMELINE: *chunks = the chunks that
 * completed; h_ms (5 floats per chunk, room for cap chunks) = H2D, decode (dictionary sync, offsets check, kernel,
 * read-back and host fallback), apply, encode, D2H milliseconds.  The call is a result-blob call of the pipeline and
 * keeps its stamps where cc_apply_batch_host_packed_results keeps its own: either timeline call reports the engine's
 * last call of either kind. */
int  cc_wire_packed_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms);

#ifdef __cplusplus
}
#endif
#endif /* COPYCAT_APPLY_H */
