/*
 * armada_sched.h — C ABI of the MI355X-native Armada scheduling-round hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI seam on this path; the
 * seam is the Go interface `SchedulingAlgo` (internal/scheduler/scheduling/scheduling_algo.go:43-47)
 * plus the concrete `*nodedb.NodeDb` (internal/scheduler/nodedb/nodedb.go:97-191).  Every entry
 * point below names the reference method it replaces; a cgo shim binds them 1:1.
 *
 * Two libraries export this ABI:
 *   - armada_amd/csrc/libarmada_sched.so   (prefix asched_)  HIP/gfx950 implementation — the product.
 *   - oracle/liboracle.so                  (prefix oracle_)  CPU restatement — TEST INFRASTRUCTURE ONLY.
 * Both are generated from this one header through ASCHED_FN(), so signatures cannot drift.
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types.  All input buffers are borrowed for the call.
 *   - return value: 0 = ok, <0 = error (asched_last_error() gives text).  "no feasible node" is a
 *     normal result (node = -1), exactly like the reference's (nil, nil, nil) (nodedb.go:629).
 *   - one thread per handle; handles are independent (NodeDb is not goroutine-safe either).
 *   - strings never cross the boundary: queue names, node ids, label/taint keys and values are
 *     interned by the caller into dense int32 ids; where the reference orders by string
 *     (queue name: queue_scheduler.go:797, scheduling.go:284; node id: nodeiteration.go:184) the
 *     caller passes the *rank* of the string in lexicographic order.
 *   - resource vectors are int64[R] in ResourceListFactory column order
 *     (internaltypes/resource_list_factory.go:41-52), row-major [n][R] at the boundary.
 */
#ifndef ARMADA_SCHED_H
#define ARMADA_SCHED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef ASCHED_PREFIX
#define ASCHED_PREFIX asched_
#endif
#define ASCHED_CAT2(a, b) a##b
#define ASCHED_CAT(a, b) ASCHED_CAT2(a, b)
#define ASCHED_FN(name) ASCHED_CAT(ASCHED_PREFIX, name)

#define ASCHED_MAX_RESOURCES 8
#define ASCHED_MAX_INDEXED 6
#define ASCHED_MAX_PRIORITIES 16

/* NodeDb-internal priorities (internaltypes/node.go:17-28). */
#define ASCHED_EVICTED_PRIORITY (-2)
#define ASCHED_CROSS_POOL_PRIORITY (-1)
#define ASCHED_MIN_PRIORITY ASCHED_EVICTED_PRIORITY

/* error codes */
#define ASCHED_OK 0
#define ASCHED_ERR_INVALID (-1)      /* bad argument / inconsistent input */
#define ASCHED_ERR_UNSUPPORTED (-2)  /* feature of the reference not implemented by this backend (the text of last_error names it: a key beyond 128 bits, more than 64 node
                                        types for one requirement class off the index grid, a batched first fit off the index grid on a two-word order key, ...) */
#define ASCHED_ERR_DEVICE (-3)       /* HIP runtime failure or no gfx950 device */
#define ASCHED_ERR_INTERNAL (-4)     /* reference would return an error here (e.g. iteration loop) */
#define ASCHED_ERR_PEER (-6)         /* a collective entry point: another rank of the communicator failed in front of the exchange (its own call returns the cause); nothing was exchanged */
#define ASCHED_ERR_TIMEOUT (-5)      /* the round's context was done: hard timeout or cancel (queue_scheduler.go:105-112 returns ctx.Err()); no result */

/* taint effects / toleration operators (k8s core/v1), interned */
#define ASCHED_EFFECT_NONE 0
#define ASCHED_EFFECT_NO_SCHEDULE 1
#define ASCHED_EFFECT_PREFER_NO_SCHEDULE 2
#define ASCHED_EFFECT_NO_EXECUTE 3
#define ASCHED_TOLERATION_OP_EQUAL 0 /* also the empty operator */
#define ASCHED_TOLERATION_OP_EXISTS 1

/* context.SchedulingType (scheduling/context/pod.go:13-21) */
#define ASCHED_METHOD_NONE 0
#define ASCHED_METHOD_RESCHEDULED 1
#define ASCHED_METHOD_NO_PREEMPTION 2
#define ASCHED_METHOD_FAIRSHARE 3
#define ASCHED_METHOD_URGENCY 4
#define ASCHED_METHOD_AWAY 5
#define ASCHED_METHOD_OPTIMISER 6 /* ScheduledWithFairnessOptimiser (the experimental fairness optimiser, optimiser/gang_scheduler.go:240) */

/* unschedulable / termination reasons (scheduling/constraints/constraints.go:25-58) */
#define ASCHED_REASON_NONE 0
#define ASCHED_REASON_MAX_RESOURCES_SCHEDULED 1      /* terminal */
#define ASCHED_REASON_MAX_RESOURCES_PER_QUEUE 2
#define ASCHED_REASON_GLOBAL_RATE_LIMIT 3            /* terminal */
#define ASCHED_REASON_QUEUE_RATE_LIMIT 4             /* queue-terminal */
#define ASCHED_REASON_QUEUE_CORDONED 5               /* queue-terminal */
#define ASCHED_REASON_GLOBAL_RATE_LIMIT_BY_GANG 6
#define ASCHED_REASON_QUEUE_RATE_LIMIT_BY_GANG 7
#define ASCHED_REASON_GANG_EXCEEDS_GLOBAL_BURST 8
#define ASCHED_REASON_GANG_EXCEEDS_QUEUE_BURST 9
#define ASCHED_REASON_GANG_DOES_NOT_FIT 10
#define ASCHED_REASON_JOB_DOES_NOT_FIT 11
#define ASCHED_REASON_RESOURCE_LIMIT_EXCEEDED 12
#define ASCHED_REASON_UNIFORMITY_LABEL_NOT_INDEXED 13
#define ASCHED_REASON_NO_NODES_WITH_UNIFORMITY_LABEL 14
#define ASCHED_REASON_GANG_UNIFORMITY_NO_FIT 15      /* "at least one job in the gang does not fit on any node" */
#define ASCHED_REASON_NO_REMAINING_CANDIDATES 16      /* sctx.TerminationReason default, queue_scheduler.go:289-291 */
#define ASCHED_REASON_SKIPPED_UNFEASIBLE_KEY 17       /* copied from the first failed job of the key, queue_scheduler.go:398-413 */
#define ASCHED_REASON_GLOBAL_NEW_JOB_DURATION 18      /* terminal: "global new job scheduling duration exceeded" (constraints.go:39,159-163) */
#define ASCHED_REASON_QUEUE_NEW_JOB_DURATION 19       /* queue-terminal: "queue new job scheduling duration exceeded" (constraints.go:40,165-169) */
#define ASCHED_REASON_FLOATING_NOT_CONFIGURED 20      /* "floating resources not configured for pool" (floating_resource_types.go:62-64) */
#define ASCHED_REASON_FLOATING_EXCEEDED 21            /* "not enough floating resource ... in pool" (floating_resource_types.go:66-69) */

typedef struct asched asched_t;

/* ---- configuration: the subset of configuration.SchedulingConfig that changes hot-path results
 *      (internal/scheduler/configuration/configuration.go:169-350; SURVEY.md §5 "Config / flags") ---- */
typedef struct asched_config {
  int32_t num_resources;              /* R = len(supportedResourceTypes)+floating */
  int32_t num_indexed;                /* K = len(indexedResources), config order (nodedb.go:204) */
  const int32_t* indexed_col;         /* [K] column of each indexed resource */
  const int64_t* indexed_resolution;  /* [K] nodedb.go:274-295, in factory units */

  int32_t num_priority_classes;       /* types.PriorityClass (internal/common/types/scheduling.go:56-76) */
  const int32_t* pc_priority;         /* [npc] */
  const uint8_t* pc_preemptible;      /* [npc] */
  const int32_t* pc_away_off;         /* [npc+1] CSR into away_* (may be NULL: no away node types) */
  const int32_t* away_priority;       /* AwayNodeType.Priority */
  const int32_t* away_well_known;     /* AwayNodeType.WellKnownNodeTypeName as index into wkt_*; -1 = "" (only NodeTypes entries) */
  int32_t num_well_known_types;       /* configuration.WellKnownNodeType */
  const int32_t* wkt_taint_off;       /* [nwkt+1] */
  const int32_t* wkt_taint_key;
  const int32_t* wkt_taint_value;     /* -1 = wildcard "*" (configuration.WildCardWellKnownNodeTypeValue) */
  const int32_t* wkt_taint_effect;

  const double* drf_multiplier;       /* [R] fairness.go:69-89 (1 for considered resources, 0 otherwise) */

  int32_t num_indexed_taints;         /* -1: index all taints (node_type.go:77-86) */
  const int32_t* indexed_taint_keys;
  int32_t num_indexed_labels;         /* node_type.go:101-109; 0: index none */
  const int32_t* indexed_label_keys;

  uint8_t prefer_large_job_ordering;  /* EnablePreferLargeJobOrdering */
  uint8_t protect_uncapped_adjusted_fair_share;
  uint8_t disable_home_scheduling, disable_away_scheduling, disable_gang_away_scheduling;
  uint8_t disable_fairshare_scheduling, disable_urgency_scheduling;
  uint8_t preempt_cross_pool_jobs_first;  /* PreemptCrossPoolJobsFirst: gangs of home jobs order before gangs of cross-pool away jobs, in the scheduling loop and
                                             in the eviction-order replay (queue_scheduler.go:744-746; pqs.go:603-606).  Away jobs: asched_jobs.away */
  double protected_fraction_of_fair_share;
  uint32_t max_queue_lookback;        /* 0 = unlimited (queue_scheduler.go:434-444) */
  uint32_t pad2_;
  const double* max_fraction_to_schedule; /* [R] MaximumResourceFractionToSchedule, +Inf = uncapped; NULL = all +Inf */
  const uint8_t* disallowed_resource;     /* [R] pool ExperimentalUnscheduledResources; NULL = none */
  int32_t device;                         /* HIP device ordinal this handle (one pool) lives on; <0 = the calling thread's current device */
  int32_t pad3_;
  /* AwayNodeType.NodeTypes (types.AwayTypeEntry, internal/common/types/scheduling.go:29-51): further well-known node types whose
     taints an away attempt tolerates when the entry's conditions hold for the job's requests (getEffectiveAwayNodeTaints,
     nodedb.go:650-675).  All optional: away_nt_off == NULL means no entry has NodeTypes. */
  const int32_t* away_nt_off;             /* [number of away entries + 1] CSR over the away entries (the order of away_priority) */
  const int32_t* away_nt_well_known;      /* AwayTypeEntry.Name as index into wkt_* */
  const int32_t* away_nt_cond_off;        /* [number of NodeTypes entries + 1] CSR: AwayTypeEntry.Conditions */
  const int32_t* away_cond_resource;      /* AwayNodeTypeCondition.Resource as column; -1 = not a resource of the factory (reads 0) */
  const int32_t* away_cond_op;            /* ASCHED_AWAY_COND_* ; any other value = an operator matchesCondition does not know */
  const int64_t* away_cond_value;         /* c.Value.Value(): whole units, rounded up */
  const int64_t* resource_unit;           /* [R] factory units per whole unit (cpu: 1000, memory: 1) — jobVal.Value() rounds up to whole
                                             units (nodedb.go:634-635); NULL = 1 for every resource */
  /* Floating resources (configuration.FloatingResourceConfig, floatingresources/floating_resource_types.go): pool-level quantities that are
     not on nodes.  [R]: the pool's total for a floating column (>= 0), -1 for an ordinary (Kubernetes) resource; NULL = none.  Job requests
     on a floating column count in every scheduling-context sum (AllResourceRequirements) and never constrain a node
     (KubernetesResourceRequirements, nodematching.go:184,195); GangScheduler.Schedule checks sctx.Allocated against the limit
     (gang_scheduler.go:143, context/scheduling.go:574-597).  A floating column cannot be indexed. */
  const int64_t* floating_resource_limit;
  uint8_t floating_counts_in_total;       /* 1: sctx.TotalResources = NodeDb total + floating totals (scheduling_algo.go:890); 0: NodeDb total only */
  uint8_t pad4_[7];
  /* Soft time budgets (constraints.go:159-169; configuration.go:190-209 MaxNewJobSchedulingDuration[PerQueue]); 0 = off.  Time spent on
     gangs of new jobs is accumulated per round and per queue (queue_scheduler.go:222-228) from the device's wall clock; clock_step_ns > 0
     replaces the clock by one that advances clock_step_ns per reading (testfixtures.SteppingClock, queue_scheduler_test.go:1546-1550). */
  int64_t max_new_job_scheduling_duration_ns;
  int64_t max_new_job_scheduling_duration_per_queue_ns;
  int64_t clock_step_ns;
} asched_config;

/* types.AwayNodeTypeConditionOperator (internal/common/types/scheduling.go:12-16) */
#define ASCHED_AWAY_COND_GT 0
#define ASCHED_AWAY_COND_LT 1
#define ASCHED_AWAY_COND_EQ 2

/* ---- nodes (internaltypes/node.go:32-69).  Creation order = node.index order. ---- */
typedef struct asched_nodes {
  int32_t n;
  const uint64_t* index;          /* [n] node.index (unique; node_factory.go:205-207) */
  const int32_t* id_rank;         /* [n] rank of node.id string; tie-break across node types (nodeiteration.go:184) */
  const int64_t* total;           /* [n][R] totalResources */
  const int64_t* allocatable;     /* [n][R] allocatableResources = initial AllocatableByPriority[p] for every p (node.go:79-85) */
  const int64_t* alloc_by_prio;   /* optional [n][P][R] explicit AllocatableByPriority (tests: WithUsedResourcesNodes); NULL = allocatable */
  const uint8_t* unschedulable;   /* [n] (adds the unschedulable taint, node.go:127-129) */
  const uint8_t* over_allocated;  /* [n] scheduling_algo.go:1081 */
  const int32_t* taint_off;       /* [n+1] CSR; may be NULL (no taints) */
  const int32_t* taint_key; const int32_t* taint_value; const int32_t* taint_effect;
  const int32_t* label_off;       /* [n+1] CSR; may be NULL */
  const int32_t* label_key; const int32_t* label_value;
  const int64_t* node_type_override; /* optional [n]: explicit node-type id (tests: WithNodeTypeNodes); <0 = derive from taints/labels */
} asched_nodes;

/* ---- static requirement classes: (tolerations, node selector) sets shared by many jobs.
 *      class 0 must exist; a job's scheduling key (internaltypes/podutils.go:52-72) is the
 *      equivalence class of (req class, requests, priority class) and is derived internally. ---- */
typedef struct asched_req_classes {
  int32_t n;
  const int32_t* tol_off;  /* [n+1] */
  const int32_t* tol_key;  /* -1 = empty key */
  const int32_t* tol_op;   /* ASCHED_TOLERATION_OP_* */
  const int32_t* tol_value;
  const int32_t* tol_effect; /* 0 = empty (matches all effects) */
  const int32_t* sel_off;  /* [n+1] PodRequirements.NodeSelector */
  const int32_t* sel_key; const int32_t* sel_value;
  /* PodRequirements.GetAffinityNodeSelector(): Affinity.NodeAffinity.RequiredDuringSchedulingIgnoredDuringExecution, checked per node by
     NodeAffinityRequirementsMet (nodematching.go:242-255, not at node-type level :127-139).  Optional: has_affinity == NULL = no class has
     one.  Terms are ORed, the expressions of a term ANDed, a term without expressions matches no node (k8s.io/component-helpers
     v0.32.11 scheduling/corev1/nodeaffinity).  Gt / Lt compare integers: asched_set_label_value_ints tells which interned values parse.
     MatchFields is not representable: ASCHED_ERR_UNSUPPORTED. */
  const uint8_t* has_affinity;   /* [n] 0 = nil NodeSelector: every node matches */
  const int32_t* aff_term_off;   /* [n+1] CSR: NodeSelectorTerms of each class */
  const int32_t* aff_expr_off;   /* [number of terms + 1] CSR: MatchExpressions of each term */
  const int32_t* aff_expr_key;   /* interned label key */
  const int32_t* aff_expr_op;    /* ASCHED_AFFINITY_OP_* */
  const int32_t* aff_value_off;  /* [number of expressions + 1] CSR into aff_values */
  const int32_t* aff_values;     /* interned label values (In / NotIn) */
} asched_req_classes;

/* v1.NodeSelectorOperator */
#define ASCHED_AFFINITY_OP_IN 0
#define ASCHED_AFFINITY_OP_NOT_IN 1
#define ASCHED_AFFINITY_OP_EXISTS 2
#define ASCHED_AFFINITY_OP_DOES_NOT_EXIST 3
#define ASCHED_AFFINITY_OP_GT 4   /* label value and the single requirement value parsed as integers (apimachinery labels.Requirement.Matches): */
#define ASCHED_AFFINITY_OP_LT 5   /* needs asched_set_label_value_ints for both; anything that does not parse matches nothing */

/* ---- jobs: the jobdb view the round needs (jobdb/job.go accessors used on the path).
 *      Job ids are their index in this table; ROWS MUST BE IN ASCENDING JOB-ID (string) ORDER: the row is the
 *      final tie-break of SchedulingOrderCompare (jobdb/comparison.go:99-105), of MarketSchedulingOrderCompare
 *      (:160-168) and of the pricer's victim order (pricer/node_scheduler.go priceOrder.Less) — the library never
 *      sees the strings, so it cannot check this; integration/gpu_round.go sorts before it uploads. ---- */
typedef struct asched_jobs {
  int32_t m;
  const int32_t* queue;            /* [m] queue index */
  const int32_t* pc;               /* [m] priority class index */
  const uint32_t* queue_priority;  /* [m] per-queue job priority (comparison.go:74-79) */
  const int64_t* submit_time;      /* [m] comparison.go:92-97 */
  const int64_t* req;              /* [m][R] AllResourceRequirements; floating columns (asched_config.floating_resource_limit) never reach a node */
  const int32_t* req_class;        /* [m] index into asched_req_classes */
  const int32_t* gang_id;          /* [m] -1 = not in a gang; ids are unique per (queue, gang) */
  const int32_t* gang_cardinality; /* [m] */
  const int32_t* gang_uniformity_label; /* [m] interned label key, -1 = none */
  const int32_t* node;             /* [m] node (position in asched_nodes) of the active run, -1 = queued */
  const int32_t* scheduled_at_priority; /* [m] run.ScheduledAtPriority for running jobs */
  const int64_t* run_timestamp;    /* [m] activeRunTimestamp (comparison.go:83-89) */
  const uint8_t* away;             /* [m] 1 = cross-pool away job: a running job whose latest run belongs to ANOTHER pool (context.IsHomeJob false, context/util.go:9-16);
                                      NULL = none.  Such a job skips this pool's floating-resource limits (context/scheduling.go:585-594) and, when
                                      preempt_cross_pool_jobs_first is set, is bound at CrossPoolPriority (-1) whatever its run says (bindJobToNodeInPlace,
                                      nodedb.go:1055-1068: the NodeDb is told its pool exactly then, scheduling_algo.go:759-764) and orders after home jobs; it belongs to the "<queue>-away" queue context: `queue` holds that context's index
                                      (CalculateAwayQueueName; jobiteration.go:88-94, context/scheduling.go:225-226, 412-413, 646-647).  The node evictor
                                      never evicts such a job for balancing (pqs.go:102-104: job.LatestRun().Pool() != sctx.Pool); urgency preemption and the
                                      oversubscribed evictor may take it */
  const double* bid_price;         /* [m] job.GetBidPrice(pool) as the job stands at the start of the round (jobdb/job.go:459-481: QueuedBid of a queued job, RunningBid of a
                                      running one, pricing.NonPreemptibleRunningPrice = 1e6 for a running non-preemptible job); NULL = 0 everywhere.  Read by market-driven
                                      rounds only (asched_set_market) */
} asched_jobs;

/* ---- per-queue round inputs (context.AddQueueSchedulingContext, scheduling/context/scheduling.go:114-166) ---- */
typedef struct asched_queues {
  int32_t q;
  const int32_t* name_rank;        /* [q] rank of the queue name */
  const double* weight;            /* [q] 1/priorityFactor (scheduling_algo.go:811-823) */
  const int64_t* allocated_by_pc;  /* [q][npc][R] initialAllocatedByPriorityClass; NULL = derive from running jobs */
  const int64_t* demand;           /* [q][R] constrainedDemand (and demand); NULL = derive (queued + running requests) */
  const int64_t* short_job_penalty;/* [q][R] NULL = zero */
  const uint8_t* cordoned;         /* [q] NULL = none */
  const double* pc_resource_limit_fraction; /* [q][npc][R] per-queue per-PC MaximumResourceFraction (+Inf = none); NULL = none */
  /* token buckets evaluated at the fixed instant sctx.Started (constraints.go:136-157):
     tokens = limiter.TokensAt(Started); rate_inf = limiter has rate +Inf (ReserveN is a no-op) */
  double global_tokens; int64_t global_burst; uint8_t global_rate_inf; uint8_t pad_[7];
  const double* queue_tokens;      /* [q] */
  const int64_t* queue_burst;      /* [q] */
  const uint8_t* queue_rate_inf;   /* [q] */
  uint8_t has_fairshare_preemption_limiter; uint8_t pad2_[7];
  double fairshare_preemption_tokens;
  /* per-queue queued jobs in SchedulingOrderCompare order (jobdb.QueuedJobs iterator, jobiteration.go:138-176) */
  const int32_t* queued_off;       /* [q+1] */
  const int32_t* queued_jobs;      /* job indices */
} asched_queues;

/* ---- per-job outcome of a node selection (context.PodSchedulingContext, scheduling/context/pod.go:37-58) ---- */
typedef struct asched_pod_result {
  int32_t node;                 /* -1 = none */
  int32_t scheduled_at_priority;
  int32_t preempted_at_priority;
  int32_t method;               /* ASCHED_METHOD_* */
} asched_pod_result;

/* ---- PodSchedulingContext.NumExcludedNodesByReason (scheduling/context/pod.go:51) of a job whose last node selection ended WITHOUT a node: how many
 *      nodes each reason excluded.  The reference keys the histogram by the reason's string (nodematching.go:14-125); strings never cross this
 *      boundary, so an entry carries what the string is made of and the caller formats it:
 *        IMPLICIT                "insufficient resources available": nodes the iterator never yielded (nodedb.go:566-580)
 *        UNTOLERATED_TAINT       a = key, b = value, c = effect          "taint %s=%s:%s not tolerated"
 *        MISSING_LABEL           a = label key                            "node does not match pod NodeSelector: label %s not set"
 *        UNMATCHED_LABEL         a = key, b = pod value, c = node value   "... required label %s = %s, but node has %s"
 *        UNMATCHED_AFFINITY      (the job's own node affinity)            "node does not match pod NodeAffinity %s"
 *        INSUFFICIENT_RESOURCES  a = resource column, required, available "pod requires %s %s, but only %s is available" (static: the node's total; dynamic:
 *                                                                         allocatable at the priority of the attempt, nodematching.go:161-197,257-267)
 *        DISALLOWED_RESOURCE     count = NumNodes (nodedb.go:596-601)
 *      Semantics (nodedb.go:538-630,724-789,881-928): the histogram of the LAST attempt — NodeTypesMatchingJob's per-type exclusions (:1118-1133), one reason per
 *      node the iterator yielded at the job's priority (every one of them failed), the rest as IMPLICIT; the counts add up to NumNodes (the reference's own
 *      check, queue_scheduler_test.go:676-690).  A pinned (evicted) job: its node's dynamic reason, the rest IMPLICIT.
 *      Where the reference itself is order-dependent the smallest id is reported: a node selector is a Go map (nodematching.go:216-243: the first failing label
 *      in map order), node-type taints are sorted by key STRING (node_type.go:87-97) — intern taint keys in lexicographic order for the same first taint.
 *      Not produced: for jobs that got a node (the nodes rejected before the match depend on the iterator's order: nothing is on record, 0 entries).
 *      An attempt that passed the feasibility gate and still ended without a node (nodedb.go:747-789: urgency preemption disabled) reports what the reference's map
 *      holds then: the gate's walk up to the node it stopped at, plus — fair-share preemption on — the static reason of every node the failed walk over the evicted
 *      table found room on (:996-1006; such a node may be counted twice, as in the reference). ---- */
typedef struct asched_excluded_reason {
  int32_t kind;       /* ASCHED_EXCL_* */
  int32_t a, b, c;
  int64_t required, available;
  int32_t count;
  int32_t pad_;
} asched_excluded_reason;
#define ASCHED_EXCL_IMPLICIT 0
#define ASCHED_EXCL_UNTOLERATED_TAINT 1
#define ASCHED_EXCL_MISSING_LABEL 2
#define ASCHED_EXCL_UNMATCHED_LABEL 3
#define ASCHED_EXCL_UNMATCHED_AFFINITY 4
#define ASCHED_EXCL_INSUFFICIENT_RESOURCES 5
#define ASCHED_EXCL_DISALLOWED_RESOURCE 6

/* ---- one unit of a submit check: SubmitChecker.getSchedulingResult's per-pool core (internal/scheduler/submitcheck.go:345-349):
 *      txn := nodeDb.Txn(true); ok, _, err := nodeDb.ScheduleManyWithTxn(txn, gctx); txn.Abort() ---- */
typedef struct asched_submit_result {
  int32_t ok;               /* ScheduleManyWithTxn's bool */
  int32_t scheduled_away;   /* gctx.JobSchedulingContexts[0].PodSchedulingContext.ScheduledAway (submitcheck.go:358) */
  int32_t num_schedulable;  /* members whose PodSchedulingContext.IsSuccessful() (submitcheck.go:366-371) */
  int32_t first_node;       /* node of member 0, -1 = none (diagnostic; the reference only prints it) */
} asched_submit_result;
#define ASCHED_SUBMIT_STRIP_GANG 1 /* unit flag: members checked as job.WithGangInfo(BasicJobGangInfo()) (submitcheck.go:274) */

/* ---- result of a round (scheduling.SchedulingResult, scheduling/result.go:96-107) ---- */
typedef struct asched_round_result {
  int32_t num_scheduled;        /* len(ScheduledJobs) */
  int32_t num_preempted;        /* len(PreemptedJobs) */
  int32_t termination_reason;   /* sctx.TerminationReason of the first schedule() pass */
  int32_t num_evicted_phase1;
  int32_t num_evicted_phase3;
  int32_t num_node_queries;     /* selectNodeForPodAtPriority-equivalents issued (roofline accounting) */
  int32_t num_loop_iterations;  /* QueueScheduler loop iterations over both passes */
  int32_t pad_;
  const int32_t* scheduled_job;       /* [num_scheduled] job ids, ascending */
  const int32_t* scheduled_node;      /* [num_scheduled] jctx.PodSchedulingContext.NodeId */
  const int32_t* scheduled_priority;  /* [num_scheduled] nodeDb.GetScheduledAtPriority */
  const int32_t* scheduled_method;
  const int32_t* preempted_job;       /* [num_preempted] ascending */
  const int32_t* preempted_node;      /* jctx.AssignedNode */
  const int64_t* queue_allocated_by_pc; /* [q][npc][R] qctx.AllocatedByPriorityClass after the round */
  const double* queue_fair_share;       /* [q] */
  const double* queue_demand_capped_adjusted_fair_share; /* [q] */
  const double* queue_uncapped_adjusted_fair_share;      /* [q] */
  const int32_t* job_unschedulable_reason; /* [m] ASCHED_REASON_* for jobs attempted and failed (0 otherwise) */
  double global_tokens_after;
  const double* queue_tokens_after;   /* [q] */
} asched_round_result;

/* ------------------------------------------------------------------ lifecycle */
asched_t* ASCHED_FN(create)(const asched_config* cfg);            /* nodedb.NewNodeDb (nodedb.go:193) + ConfigureScheduling (:386) */
void ASCHED_FN(destroy)(asched_t*);
const char* ASCHED_FN(last_error)(asched_t*);
/* nodedb priorities: [-2,-1]+sorted-unique(PC ∪ away priorities) (nodedb.go:201-202). Returns P. */
int32_t ASCHED_FN(priorities)(asched_t*, int32_t* out /*[ASCHED_MAX_PRIORITIES]*/);

/* ------------------------------------------------------------------ NodeDb level */
/* CreateAndInsert / UpsertMany (nodedb.go:57-75,1135-1175). Replaces all nodes. */
int32_t ASCHED_FN(nodes_upsert)(asched_t*, const asched_nodes* nodes);
/* Which interned label values are integers (strconv.ParseInt(value, 10, 64) succeeds) and their value — what the Gt / Lt node-affinity
   operators compare (k8s.io/apimachinery labels.Requirement.Matches: both sides must parse, exactly one requirement value).  Replaces the
   table; call before jobs_set / nodes_upsert evaluate affinities (the static masks are rebuilt by whichever of the two comes last). */
int32_t ASCHED_FN(set_label_value_ints)(asched_t*, int32_t n, const int32_t* value_ids, const int64_t* ints);
/* registers the job + requirement tables referenced by job id in the calls below */
int32_t ASCHED_FN(jobs_set)(asched_t*, const asched_jobs* jobs, const asched_req_classes* classes);
/* jobdb.Txn.Upsert for run-state changes between two scheduling cycles: txn.Upsert(preemptedJobs) / txn.Upsert(scheduledJobs) (scheduling/scheduling_algo.go:280-283, the
   jobs built at :956-981), after which jobdb/jobdb.go:572-700 re-seats only those jobs in the per-queue sorted sets (SchedulingOrderCompare, jobdb/comparison.go:49-107).
   entry i: job[i] (row of the job table) now has its active run on node[i] at scheduled_at_priority[i], leased at run_timestamp[i] (ns);
   node[i] == -1: the job has no active run any more (preempted, finished, lease returned).  Whether such a job is queued again is, as always,
   what the queued lists of the next round_prepare say; a row that is neither running nor in a queued list takes no part in a round.
   scheduled_at_priority / run_timestamp NULL: zeros.
   After a successful call the handle is in the state asched_jobs_set would have left, given the same job table with node, scheduled_at_priority and run_timestamp
   replaced in the named rows and the same requirement classes — for every entry point, including everything jobs_set resets (the caller goes on with round_prepare).
   The work is on the device and proportional to the job order, not a rebuild: no static masks, no job-record upload, no sort of all jobs; the fast structure stays.
   n == 0 performs the resets only.  Refused before anything changes — ASCHED_ERR_INVALID: no job table, a row outside [0, M), a row named twice, a node outside
   [-1, N); ASCHED_ERR_UNSUPPORTED: the job set carries the market order (uploaded with bid prices or after asched_set_market), an entry gives a cross-pool away row
   (asched_jobs.away) a node >= 0.  On a handle without a node table N is 0: only node -1 is accepted.  ASCHED_ERR_DEVICE (a failed launch or copy, as from any
   other entry point) is NOT such a refusal: the job table may be half patched, and the handle needs asched_jobs_set before anything else.
   No other field changes (a finished job stays as a row without a run until asched_jobs_delete removes it); newly submitted rows are appended with
   asched_jobs_append. */
int32_t ASCHED_FN(jobs_patch)(asched_t*, int32_t n, const int32_t* job, const int32_t* node, const int32_t* scheduled_at_priority, const int64_t* run_timestamp);
/* The two Upserts a pool's cycle ends with (scheduling/scheduling_algo.go:276-285: txn.Upsert(preemptedJobs), txn.Upsert(scheduledJobs), the jobs of :956-981),
   taken from the result of the round the handle holds: the lists asched_round_result pointed at are still on the device, so the caller builds and sends no entry for
   them.  The handle must hold a round result (asched_schedule_round, and no call that changes the handle since).  After a successful call the handle is in the state
   asched_jobs_patch would leave, given this entry list in any order — the state asched_jobs_set would leave for the table with those run fields replaced — for every
   entry point, including everything jobs_patch resets (no round prepared, no result held, the state epoch, the dynamic state; the caller goes on with round_prepare):
     i in [0, num_scheduled): row scheduled_job[i] runs on scheduled_node[i] at scheduled_priority[i], leased at run_timestamp + i * run_timestamp_step (ns), i the
       position in the result's ascending list (the reference's scheduled list is maps.Values, of unspecified order: any monotone assignment is legal; step 0 gives
       every lease the cycle's time);
     i in [0, num_preempted): row preempted_job[i] has node -1, priority 0, timestamp 0;
     the n_extra entries of the caller, with jobs_patch's meaning (the other run-state changes of the cycle, such as the runs that ended): re-seated in the same
       remove / sort / merge pass.  scheduled_at_priority / run_timestamp_extra NULL: zeros.
   A round that scheduled and preempted nothing, with n_extra == 0, performs the resets only.
   READ BEFORE THE COMMIT what belongs to the round: asched_round_preemption_causes and asched_round_evictor_report are invalid afterwards, as after jobs_patch.  The
   pointers of the last asched_round_result stay readable exactly as long as they do after jobs_patch today: until the next round on the handle (the commit reads the
   lists, it does not write or free them).
   Refused before anything changes, as by jobs_patch — ASCHED_ERR_INVALID: no job table, no round result held (never run, or reset by any call since), n_extra < 0,
   n_extra > 0 without job or node, an extra row outside [0, M), an extra node outside [-1, N), an extra row named twice, an extra row that the round's scheduled or
   preempted list names (the caller sends that change with a later jobs_patch); ASCHED_ERR_UNSUPPORTED: the job set carries the market order, more than 2^29 entries
   in all, a cross-pool away row that would gain a run (from the extras or from the scheduled list), a result that asched_round_exchange has resolved against other
   replicas since (the lists are this replica's own round); ASCHED_ERR_DEVICE with "the handle is as it was" in last_error: out of device memory for the scratch.
   Any other ASCHED_ERR_DEVICE (a failed launch or copy) is NOT such a refusal: the handle then needs asched_jobs_set, as documented for jobs_patch. */
int32_t ASCHED_FN(round_commit)(asched_t*, int64_t run_timestamp, int64_t run_timestamp_step, int32_t n_extra, const int32_t* job, const int32_t* node,
                                const int32_t* scheduled_at_priority, const int64_t* run_timestamp_extra);
/* how the last round_commit ran: out[0] scheduled entries, [1] preempted entries, [2] extra entries, [3] entries that name a row in the order (queue >= 0), [4] 1 = this
   call made the order-key inputs resident (the first incremental call on the job table), [5..7] device microseconds of scatter / remove + sort / merge (measured only
   with ASCHED_JP_TIMES=1, else 0).  Zeros after jobs_set. */
int32_t ASCHED_FN(round_commit_stats)(asched_t*, int32_t* out /*[8]*/);
/* `armadactl reprioritize` for resident jobs, one job or a whole job set: jobdb/reconciliation.go:198-200 records the requested priority, scheduler.go:1198-1199
   applies it (job.WithPriority(job.RequestedPriority()), jobdb/job.go:523), and Txn.Upsert takes the job out of its queue's sorted set and puts it back under the new
   key (jobdb/jobdb.go:583-587, :695-699); the queue priority is the second word of that key (SchedulingOrderCompare, jobdb/comparison.go:70-79).
   entry i: job[i] (row of the job table) now has queue_priority[i]; any uint32 value, 0 and 0xFFFFFFFF included.  Any row may be named: queued or running (the active
   group of a queue is ordered by priority class, queue priority, run timestamp), a gang member, a cross-pool away row, a row of queue -1 (its stored priority changes
   and it stays in no order).  An entry that repeats the row's current priority is legal and leaves the row where it is.
   After a successful call the handle is in the state asched_jobs_set would have left, given the same job table with queue_priority replaced in the named rows and the
   same requirement classes — for every entry point (rounds after either form of round_prepare, scheduling_order, round_queued, the NodeDb-level calls, the submit
   check, the optimiser, a later jobs_patch / jobs_append / jobs_delete / nodes_* / req_classes_append in any order), including everything jobs_set and jobs_patch
   reset; the caller goes on with round_prepare.  n == 0 performs the resets only.  Only the pre-sorted order depends on the queue priority: the work is on the device
   and proportional to the job order — no static masks, no job-record upload, no sort of all jobs, no segment offset changes; the fast structure stays.
   Refused before anything changes — ASCHED_ERR_INVALID: no job table, n < 0, n > 0 without job or queue_priority, a row outside [0, M), a row named twice;
   ASCHED_ERR_UNSUPPORTED: the job set carries the market order, more than 2^29 entries; ASCHED_ERR_DEVICE with "the handle is as it was" in last_error: out of device
   memory for the scratch.  Any other ASCHED_ERR_DEVICE (a failed launch or copy) is NOT such a refusal: the handle then needs asched_jobs_set, as documented for
   jobs_patch.  No other field changes: queue, priority class, submit time and gang of a row are fixed for as long as it is in the table; its requirement class and
   request change only through asched_jobs_respec. */
int32_t ASCHED_FN(jobs_reprioritise)(asched_t*, int32_t n, const int32_t* job, const uint32_t* queue_priority);
/* how the last jobs_reprioritise ran: out[0] entries, [1] entries that name a row in the order (queue >= 0), [2] entries whose priority did not change, [3] 1 = this
   call made the order-key inputs resident (the first incremental call on the job table), [4..7] device microseconds of scatter / remove / sort / merge (measured only
   with ASCHED_JP_TIMES=1, else 0).  Zeros after jobs_set. */
int32_t ASCHED_FN(jobs_reprioritise_stats)(asched_t*, int32_t* out /*[8]*/);
/* A retry of resident jobs: when a run fails and the job is requeued, the reference rewrites its scheduling requirements before it re-enters its queue
   (scheduler.go:1342-1383, through job.WithJobSchedulingInfo): node anti-affinity for every attempted run (createSchedulingInfoWithNodeAntiAffinityForAttemptedRuns,
   :637-658, adopted at :1369-1376) — a new (tolerations, selector, affinity) set, here a new requirement class — and the retry policy's memory bump
   (createSchedulingInfoWithMemoryBump, :683 ff., adopted at :1347-1354) — a new request vector, here a new scheduling-key shape.  The job keeps its id, queue, priority
   class, submit time and gang.
   entry i: row job[i] now has requirement class req_class[i] (NULL: every class unchanged) and the request req[i][R] (NULL: every request unchanged).  A new class is
   brought first with asched_req_classes_append; req_class[i] must be below the handle's number of real classes.  Accepted rows are rows without a run: of any queue
   >= -1, gang members, with any request vector — off the index grid, or one no node holds.  An entry equal to the row's current (class, request) is legal and changes
   nothing.  The pre-sorted order depends on neither field, so nothing is sorted or merged; a shape the table does not hold, or holds without a row, takes the path it
   takes in asched_jobs_append (in place with asched_set_append_in_place where its conditions hold, else the rebuild; asched_jobs_respec_stats says which and why).  A
   shape that loses its last row stays known, as after asched_jobs_delete, until asched_shapes_compact.
   After a successful call the handle is in the state asched_jobs_set would have left, given the same job table with req_class and req replaced in the named rows and
   the same class list — for every entry point (rounds after either form of round_prepare, scheduling_order, round_queued, fit_select_batch, node_types_matching_job,
   the submit check, job_key_unfeasible, the optimiser, any later resident call in any order), including everything jobs_set and jobs_patch reset; shape ids and dead
   shapes are not observable.  n == 0 performs the resets only.
   Refused before anything changes — ASCHED_ERR_INVALID: no job table, n < 0, n > 0 with both arrays NULL or without job, a row outside [0, M), a row named twice, a
   class out of range, a row that has a run (the caller ends the run with asched_jobs_patch first, in syncState's order); ASCHED_ERR_UNSUPPORTED: the job set carries
   the market order, a cross-pool away row, more than 2^29 entries, whatever the rebuild for a new shape would refuse (an order key beyond 128 bits, LIT_TMAX);
   ASCHED_ERR_DEVICE with "the handle is as it was" in last_error: out of device memory for the scratch or the staged blocks.  Any other ASCHED_ERR_DEVICE is NOT such
   a refusal: the handle then needs asched_jobs_set, as documented for jobs_patch. */
int32_t ASCHED_FN(jobs_respec)(asched_t*, int32_t n, const int32_t* job /*[n] rows, each at most once*/, const int32_t* req_class /*[n] or NULL: unchanged*/,
                               const int64_t* req /*[n][R] or NULL: unchanged*/);
/* how the last jobs_respec ran: out[0] entries, [1] entries that changed nothing, [2] new shapes, [3] revived shapes (known, without a row before the call), [4] shapes
   this call left without a row, [5] 1 = masks and fast structure were rebuilt, [6] the reason code of asched_jobs_append_shape_stats (0 = in place or nothing to
   grow), [7] records written from templates.  Zeros after jobs_set. */
int32_t ASCHED_FN(jobs_respec_stats)(asched_t*, int32_t* out /*[8]*/);
/* syncState's upsert of the newly submitted jobs into the jobDb at the start of a cycle (scheduler.go:478-535; jobdb/jobdb.go:572-700, the insertion into the per-queue
   sorted set at :691-700): rows->m rows are added behind the M rows the handle holds; the new job ids are M .. M+m-1.  Rows must stay in ascending job-id order, as for
   jobs_set (newly submitted ULIDs sort after the resident ones; the caller sorts the batch).  The requirement classes are those of the last jobs_set.
   After a successful call the handle is in the state asched_jobs_set would have left, given the concatenated table and the same requirement classes — for every entry
   point (rounds, scheduling_order, the NodeDb-level calls, the submit check, the optimiser, a later jobs_patch that names old and new rows), including everything jobs_set
   and jobs_patch reset; the caller goes on with round_prepare.  m == 0 performs the resets only.
   Accepted rows: queued jobs only (node NULL or all -1; scheduled_at_priority / run_timestamp NULL or 0; away NULL or 0; bid_price NULL); any queue index >= -1, a
   queue the table has no job of and an index above every earlier one included; any priority class; req_class below the table's number of classes; a gang member only
   when its (queue, gang_id) is not in the table yet — a gang is submitted in one piece, and new gangs get the next dense ids in order of first occurrence; any request
   vector.  Where every row's scheduling-key shape (req_class, pc, req) is already in the table the work is on the device and proportional to the batch and the job
   order: no static masks, no job-record upload, the fast structure stays.  A row with a new shape gets the next shape id and the shape-dependent tables (key layout,
   masks, fast structure) are rebuilt as jobs_set builds them.  The per-job device arrays have a capacity: an append that does not fit moves them to blocks of
   max(M + m, 1.25 x capacity) rows; a handle that never appends allocates exactly M.
   Refused before anything changes — ASCHED_ERR_INVALID: no job table, m < 0, req missing, req_class or pc out of range, a queue below -1, a row with a run, a row flagged
   away; ASCHED_ERR_UNSUPPORTED: the job set carries the market order, bid_price is given, a row joins a gang that already has rows in the table, M + m exceeds 2^30,
   whatever the rebuild for a new shape would refuse (a key beyond 128 bits, more than LIT_TMAX node types on the literal path); ASCHED_ERR_DEVICE with "the handle is as
   it was" in last_error: out of device memory while sizing the new blocks.  Any other ASCHED_ERR_DEVICE (a failed launch or copy) is NOT such a refusal: the handle
   then needs asched_jobs_set, as documented for jobs_patch. */
int32_t ASCHED_FN(jobs_append)(asched_t*, const asched_jobs* rows);
/* how the last jobs_append ran: out[0] rows of the call, [1] rows that entered the order (queue >= 0), [2] new shapes, [3] new gangs, [4] 1 = the per-job arrays were
   re-allocated, [5] 1 = masks and fast structure were rebuilt (0 after an in-place append of new shapes), [6] capacity (rows) after the call, [7] shapes served in
   place, new plus revived (asched_set_append_in_place).  Zeros after jobs_set. */
int32_t ASCHED_FN(jobs_append_stats)(asched_t*, int32_t* out /*[8]*/);
/* New shapes without a rebuild.  A scheduling-key shape is the whole request vector, so most cycles of a production pool bring one; with the switch on, a
   jobs_append whose rows bring new shapes — or shapes asched_jobs_delete left without a resident row — grows the shape-dependent tables by what those shapes add
   instead of re-deriving them for every shape: the new rows of the shape mask on the device (one wave per 64-node word), the rows of a newly derived away class,
   the new fit shapes, the two minima of the fast structure, and one record template per shape from which the device fills the new rows' records.  No resident row's
   record, no resident mask row and no class is recomputed or uploaded.  The handle is left as jobs_set of the concatenated table would leave it, as for every
   jobs_append; the result is the same with the switch on or off.  The path is taken where (a) the handle has a node table and masks, (b) the key layout layoutKeys
   chooses for the grown table is the one in force, (c) the batch does not bring the first away rows of the table, (d) the fit shapes still number at most SMAX,
   (e) no request of the batch is negative on a handle with the fast structure or the fused level pass, (f) the table had rows and shapes before the call; otherwise
   the rebuild of jobs_append runs and asched_jobs_append_shape_stats says why.  A handle without the fast structure (two-word keys, alloc_by_prio, ...) takes the
   mask part only.  A property of the handle like asched_set_evictor_report: off by default, survives jobs_set and nodes_upsert.  Off, jobs_append is unchanged. */
int32_t ASCHED_FN(set_append_in_place)(asched_t*, int32_t on);
/* how the last jobs_append treated new shapes: out[0] the switch, [1] shapes added in place, [2] shapes revived in place, [3] mask rows added (shape rows + away
   rows), [4] derived away classes added, [5] fit shapes F after the call, [6] why the rebuild was taken although the switch is on — 0 not taken, 1 no node table or no
   masks yet, 2 the key layout of the grown table differs, 3 the batch turns away rows on for a table that had none, 4 more than SMAX fit shapes, 5 a negative
   request on a handle with the fast structure, 6 the table had no rows or shapes — [7] 0 (reserved).  [1..7] are zero after jobs_set; [0] is always the switch. */
int32_t ASCHED_FN(jobs_append_shape_stats)(asched_t*, int32_t* out /*[8]*/);
/* New requirement classes without jobs_set.  A submission whose (tolerations, node selector, required node affinity) set the table has not seen — a new node
   selector, a pin to a hostname, a new toleration — brings a requirement class: the selector / toleration / affinity part of the scheduling key
   (internaltypes/podutils.go:52-72), which syncState's upsert of the new jobs (scheduler.go:539-549) carries into the jobDb.  `more` has the layout jobs_set takes;
   its more->n classes get the ids C .. C + n - 1 behind the C resident real classes (C >= 1: a jobs_set without classes has the empty class 0), in their order.
   Returns 0.  The handle is left as jobs_set of the same job table with the concatenated class list would leave it, including everything jobs_set resets (what
   jobs_append resets for no rows; n == 0 performs the resets only); go on with jobs_append of the rows that name the new classes, or round_prepare.
   No resident row names a new class, so shapes, shape mask, fit shapes, key layout and job records stay.  The class mask grows by n rows in a fresh block: the
   resident rows are copied device to device, the derived away classes behind C move up by n, and a new row is decided by node type on the device (the OR of the
   node-type mask rows of the types the class matches) where the class has no required affinity, every selector key is an indexed label key, every taint a
   resident node carries is indexed and the node table came without node_type_override; otherwise the host matches it node by node and uploads the row.  Where
   the fast structure exists every node gains the bits of the new classes that match it.  Where that cannot be exact the tail of jobs_set runs on the grown class
   list and asched_req_classes_append_stats gives the reason; the result is the same.  A handle without the fast structure takes the mask part only.
   Refused before anything changes: no job table, more == NULL, n < 0, a CSR offset array that is missing where its values are given or that is not ascending,
   has_affinity without the term arrays (ASCHED_ERR_INVALID); an unknown affinity operator, a job set that carries the market order (ASCHED_ERR_UNSUPPORTED); no
   device memory for the fresh class mask (ASCHED_ERR_DEVICE, the handle is as it was).  A launch or copy that fails later is ASCHED_ERR_DEVICE and the handle
   then needs asched_jobs_set, as documented for jobs_patch. */
int32_t ASCHED_FN(req_classes_append)(asched_t*, const asched_req_classes* more);
/* how the last req_classes_append ran: out[0] classes added, [1] rows decided by node type on the device, [2] rows matched on the host, [3] derived rows moved,
   [4] 1 = masks and fast structure were rebuilt, [5] why — 0 not rebuilt, 1 no node table or no masks yet (the classes are kept on the host and the next
   nodes_upsert builds everything), 2 the call takes C from at most 64 to more than 64 on a handle with the fast structure — [6] C after the call, [7] C plus the
   derived away classes after the call.  Zeros after jobs_set. */
int32_t ASCHED_FN(req_classes_append_stats)(asched_t*, int32_t* out /*[8]*/);
/* Retire the scheduling-key shapes and requirement classes no resident row names.  jobs_delete keeps an emptied shape's id, mask rows and fit shape, the in-place
   append only adds shapes and classes are append-only, while the fast structure needs at most SMAX (256) fit shapes and 64 real classes and the split node engine at
   most 128 fit shapes: on a handle that stays resident the dead ones alone reach those limits.  A shape is dead when no resident row has it, a fit shape when no
   live shape maps to it, a real class (only with ASCHED_COMPACT_CLASSES) when no live shape names it.  The live ones keep their relative order and get dense ids:
   new id = old id - number of dead ones below it.  With ASCHED_COMPACT_CLASSES class_new_id, when not NULL, receives that map for the C classes the handle had
   before the call, -1 for a retired class: rows of a later jobs_append and the classes of a later req_classes_append use the new ids.  Without the flag classes and
   their ids stay and class_new_id is ignored.
   Returns 0.  The handle is left as jobs_set of the same job table (with the class list reduced to the live classes and req_class renumbered, where classes were
   retired) would leave it, for every entry point and including everything jobs_set resets; go on with round_prepare or any other resident call.  Results equal the
   fresh handle's; internal shape ids need not.  The key layout, the two minima, hasAway, the gang tables and the capacities stay: bounds and unions over rows and
   shapes, which fewer shapes can only make tighter.  Nothing dead performs the resets only.
   In place where the handle has masks: the rows' shape ids and job records are remapped on the device, the mask rows gathered into fresh blocks, the class bits
   of every node compacted; no mask is matched again and no job record uploaded.  Where the compaction makes the fast structure possible again (F from above SMAX
   to at most SMAX, or C from above 64 to at most 64, on a handle that otherwise qualifies), and where there are no masks yet, the tail of jobs_set runs on the
   compacted tables; asched_shapes_compact_stats says which.
   Refused before anything changes: no job table, unknown flag bits (ASCHED_ERR_INVALID); a job set that carries the market order, a table with no rows
   (ASCHED_ERR_UNSUPPORTED); no device memory for the fresh blocks (ASCHED_ERR_DEVICE, the handle is as it was).  A launch or copy that fails later is
   ASCHED_ERR_DEVICE and the handle then needs asched_jobs_set, as documented for jobs_patch. */
#define ASCHED_COMPACT_CLASSES    1   /* also retire requirement classes that no remaining shape names */
#define ASCHED_COMPACT_COUNT_ONLY 2   /* change nothing: fill the statistics only (O(S) on the host) */
int32_t ASCHED_FN(shapes_compact)(asched_t*, int32_t flags, int32_t* class_new_id /* [C before the call] or NULL */);
/* how the last shapes_compact ran: out[0] shapes retired, [1] fit shapes retired, [2] real classes retired, [3] derived away classes after the call, [4] 1 = masks
   and fast structure were rebuilt, [5] why — 0 not rebuilt, 1 no node table or no masks yet, 2 F came back under SMAX, 3 C came back under 65 — [6] shapes S after
   the call, [7] fit shapes F after the call.  After ASCHED_COMPACT_COUNT_ONLY: [0..2] what a call with the same flags would retire, [6..7] the current values.
   Zeros after jobs_set. */
int32_t ASCHED_FN(shapes_compact_stats)(asched_t*, int32_t* out /*[8]*/);
/* syncState's delete of the jobs in a terminal state from the jobDb, after the upserts of the same cycle (scheduler.go:539-549; Txn.BatchDelete / delete,
   jobdb/jobdb.go:941-990): the n rows job[0..n) leave the table.  The remaining rows keep their order and are renumbered densely: new id = old id - number of
   deleted rows below it.  new_id, when not NULL, receives that map for the M rows the table had before the call, -1 for a deleted row.
   After a successful call the handle is in the state asched_jobs_set would have left, given the same table without the named rows and the same requirement classes —
   for every entry point (rounds, scheduling_order, the NodeDb-level calls, the submit check, the optimiser, the preemption causes, the evictor report, a later
   jobs_patch / jobs_append / nodes_patch in any order), including everything jobs_set resets; the caller goes on with round_prepare.  n == 0 performs the resets only.
   Any row may be named: queued, running, away, a gang member (the reference deletes gang members one by one, jobdb.go:978-990: the gang goes on with the members it
   has left; once the last one is gone its (queue, gang_id) may be appended again as a new gang).  The work is on the device and proportional to the table: every
   static per-job array is moved, the order and the gang lists are compacted; no static masks, no job-record upload, no sort, the fast structure stays.  Capacities do
   not shrink.  A scheduling-key shape that loses its last row stays known; a later jobs_append that brings it again takes the rebuild path of a new shape.
   Naming EVERY row is refused (ASCHED_ERR_UNSUPPORTED): a table without rows is not something this call leaves behind — give the next table to asched_jobs_set.
   Refused before anything changes — ASCHED_ERR_INVALID: no job table, n < 0, n > 0 without job, a row outside [0, M), a row named twice; ASCHED_ERR_UNSUPPORTED: the
   job set carries the market order, every row is named; ASCHED_ERR_DEVICE with "the handle is as it was" in last_error: out of device memory for the scratch and the
   compacted arrays (all of it is allocated first).  Any other ASCHED_ERR_DEVICE (a failed launch or copy) is NOT such a refusal: the handle then needs
   asched_jobs_set, as documented for jobs_patch. */
int32_t ASCHED_FN(jobs_delete)(asched_t*, int32_t n, const int32_t* job /*[n] rows, each at most once*/, int32_t* new_id /*[M before the call] or NULL*/);
/* how the last jobs_delete ran: out[0] rows deleted, [1] rows that left the order (queue >= 0), [2] gangs emptied, [3] scheduling-key shapes emptied, [4] M after the
   call, [5] capacity (rows), [6..7] 0 (reserved).  Zeros after jobs_set. */
int32_t ASCHED_FN(jobs_delete_stats)(asched_t*, int32_t* out /*[8]*/);
/* the per-cycle changes of resident nodes (populateNodeDb, scheduling_algo.go:1069-1095: IsUnschedulable, WithOverAllocated,
   MarkResourceUnallocatable; a changed taint set) */
typedef struct asched_nodes_patch_rows {
  int32_t n;
  const int32_t* node;            /* [n] position in the node table, each named at most once */
  const int64_t* allocatable;     /* [n][R] or NULL = unchanged */
  const uint8_t* unschedulable;   /* [n] or NULL = unchanged */
  const uint8_t* over_allocated;  /* [n] or NULL = unchanged */
  const int32_t* taint_off;       /* [n+1] CSR or NULL = taints unchanged (the unschedulable taint is never listed: the library adds it) */
  const int32_t* taint_key; const int32_t* taint_value; const int32_t* taint_effect;
} asched_nodes_patch_rows;
/* The node table of the last nodes_upsert with the named fields replaced in the named rows: cordon and uncordon, WithOverAllocated, allocatable after
   MarkResourceUnallocatable, a changed taint set — what populateNodeDb re-reads per node every cycle.
   After a successful call every entry point answers as it would after asched_nodes_upsert of that table (rounds, the NodeDb-level calls, fit_select_batch, submit_check,
   iterate_nodes, excluded_nodes, node_types_matching_job, num_nodes, total_resources, the getters, the evictor report, the preemption causes, the optimiser), including
   everything nodes_upsert resets: no round is prepared and no round result is held, every plane equals allocatable, no job is bound (running jobs stay on a node that
   becomes unschedulable: round_prepare binds them as always).  The job table, the requirement classes and the fast structure stay; the caller goes on with round_prepare.
   n == 0 performs the resets only.
   Two paths, chosen per call (nodes_patch_stats).  Where every patched row's new node type is one the table already has, no type gains its first or loses its last node
   and every new allocatable value lies inside what the key layout of the table was sized for (within [0, total]; on an indexed column not above the table's largest
   value, a multiple of the key's divisor, and a multiple of the index resolution where every resident value is one), the work is on the device and proportional to the
   entries: no host loop over all nodes, no mask rebuild, no job-record upload.  Otherwise the patched table goes through nodes_upsert's own code.
   Refused before anything changes — ASCHED_ERR_INVALID: no node table, n < 0, n > 0 without node, a node outside [0, N), a node named twice, a taint_off that is not
   ascending; ASCHED_ERR_UNSUPPORTED: the table was uploaded with alloc_by_prio or node_type_override (test-fixture inputs), whatever the rebuild would refuse (a key
   beyond 128 bits, more than LIT_TMAX node types on the literal path); ASCHED_ERR_DEVICE with "the handle is as it was" in last_error: out of device memory for the
   entries.  Any other ASCHED_ERR_DEVICE (a failed launch or copy) is NOT such a refusal: the handle then needs asched_nodes_upsert.
   Not this call's job: removing rows is asched_nodes_delete's (the reference's dropping of an unschedulable node that holds no job, scheduling_algo.go:1070-1077);
   adding rows is asched_nodes_append's; total, labels, index and id_rank of resident rows are asched_nodes_upsert's. */
int32_t ASCHED_FN(nodes_patch)(asched_t*, const asched_nodes_patch_rows* rows);
/* how the last nodes_patch ran: out[0] entries, [1] rows whose node type changed, [2] 1 = the rebuild path ran, [3] why: 0 none, 1 a node type the table did not
   have, 2 a node type emptied or newly populated, 3 key layout / divisor / alignment; [4..7] 0.  Zeros after nodes_upsert. */
int32_t ASCHED_FN(nodes_patch_stats)(asched_t*, int32_t* out /*[8]*/);
/* populateNodeDb leaves a node that IsUnschedulable() and holds no job out of the NodeDb, "so the resource of the node is not counted for fairshare"
   (scheduling_algo.go:1069-1077), and so it does with every node of an executor it filters out as stale, lagging or cordoned (:1100-1169): the n rows node[0..n)
   leave the resident node table.  The remaining rows keep their order and are renumbered densely: new position = old position - number of deleted rows below it.
   new_id, when not NULL, receives that map for the N rows the table had before the call, -1 for a deleted row.
   After a successful call every entry point answers as it would after asched_nodes_upsert of the same node table without the named rows, with the resident job table's
   runs sent through that map (rounds, the NodeDb-level calls, fit_select_batch*, submit_check, iterate_nodes, excluded_nodes, node_types_matching_job, num_nodes,
   total_resources, indexed_node_label_values, the getters, the evictor report, the preemption causes, the optimiser, a later jobs_patch / jobs_append / jobs_delete /
   nodes_patch in any order), including everything nodes_upsert resets; the caller goes on with round_prepare.  n == 0 performs the resets only.  Block sizes do not
   shrink.  The job table's rows, order, shapes, gangs and requirement classes stay, and so does the fast structure.  Aggregates that are bounds (the widths of the key
   layout, alignment, the gcd of a column) stay conservative: results equal the fresh handle's, internal widths and path choices need not.
   Two paths, chosen per call (nodes_delete_stats).  Where no node type and no value of an indexed label loses its last node, the work is on the device: the per-node
   arrays are gathered into blocks with the new stride, every mask row is bit-compacted, the index order is compacted and the running jobs' nodes are renumbered; the
   host compacts its per-node mirrors.  Otherwise the reduced table goes through nodes_upsert's own code and the jobs' nodes are renumbered on the device.
   Refused before anything changes — ASCHED_ERR_INVALID: no node table, n < 0, n > 0 without node, a row outside [0, N), a row named twice, a resident job whose run is
   on a named row (the reference logs "assigned to node ..., but no such node found" and leaves such a job unbound; here the caller says what became of the run first:
   jobs_patch with node -1, or jobs_delete; last_error names the lowest such job row); ASCHED_ERR_UNSUPPORTED: every row is named (give the next table to
   asched_nodes_upsert), the table was uploaded with alloc_by_prio or node_type_override, whatever the rebuild would refuse; ASCHED_ERR_DEVICE with "the handle is as
   it was" in last_error: out of device memory for the scratch and the fresh blocks (all of it is allocated first).  Any other ASCHED_ERR_DEVICE (a failed launch or
   copy) is NOT such a refusal: the handle then needs asched_nodes_upsert and asched_jobs_set.
   Not this call's job: adding rows (asched_nodes_append). */
int32_t ASCHED_FN(nodes_delete)(asched_t*, int32_t n, const int32_t* node /*[n] rows, each at most once*/, int32_t* new_id /*[N before the call] or NULL*/);
/* how the last nodes_delete ran: out[0] rows deleted, [1] job rows whose node was renumbered, [2] 1 = the rebuild path ran, [3] why: 0 none, 2 a node type emptied,
   4 a value of an indexed label emptied; [4] N after the call, [5..7] 0.  Zeros after nodes_upsert. */
int32_t ASCHED_FN(nodes_delete_stats)(asched_t*, int32_t* out /*[8]*/);
/* populateNodeDb inserts whatever nodes the healthy executors report (scheduling_algo.go:1019-1098): a cluster that scales up, an executor that was stale, lagging
   or cordoned and returns (:1100-1169), a drained node that is uncordoned.  The m rows join the resident node table behind the N resident ones, at positions
   N .. N + m - 1; no resident position changes, so no run of the resident job table is renumbered. */
typedef struct asched_nodes_append_rows {   /* the fields of asched_nodes, for the m new rows */
  int32_t m;
  const uint64_t* index;          /* [m] node.index: unique among the new rows and against the resident ones */
  const int32_t* id_rank;         /* [m] in the rank space of the resident rows (only the order matters); NULL = behind every resident rank, in row order */
  const int32_t* id_rank_all;     /* optional [N+m]: replaces the id rank of EVERY row (the caller re-ranked its id strings); overrides id_rank */
  const int64_t* total;           /* [m][R] */
  const int64_t* allocatable;     /* [m][R] */
  const uint8_t* unschedulable;   /* [m] or NULL */
  const uint8_t* over_allocated;  /* [m] or NULL */
  const int32_t* taint_off; const int32_t* taint_key; const int32_t* taint_value; const int32_t* taint_effect;   /* CSR or NULL */
  const int32_t* label_off; const int32_t* label_key; const int32_t* label_value;                               /* CSR or NULL */
} asched_nodes_append_rows;
/* After a successful call every entry point answers as it would after asched_nodes_upsert of the table "the N resident rows in their order, then the m new rows"
   (rounds, the NodeDb-level calls, fit_select_batch*, submit_check, iterate_nodes, excluded_nodes, node_types_matching_job, num_nodes, total_resources,
   indexed_node_label_values, the getters, the evictor report, the preemption causes, the optimiser, a later jobs_patch / jobs_append / jobs_delete / nodes_patch /
   nodes_delete in any order), including everything nodes_upsert resets; the caller goes on with round_prepare.  m == 0 performs the resets only.  A run on a new node
   is told afterwards with jobs_patch or jobs_append, naming the new position.  The job table, its order, shapes, gangs, requirement classes and the fast structure
   stay.  Aggregates that are bounds (the widths of the key layout, alignment, the gcd of a column, id order == index order) stay conservative: results equal the fresh
   handle's, internal widths and path choices need not.  Unlike a delete, an append can VIOLATE such a bound: it then takes the rebuild path.
   Id ranks: a table that asched_nodes_upsert was given WITHOUT id_rank has no rank space (its id order is its index order by definition); it takes appends without
   ranks, which keep that definition, or with id_rank_all, which gives every row a rank; id_rank alone is refused there.  m == 0 performs the resets only and ignores
   id_rank_all.
   Two paths, chosen per call (nodes_append_stats).  The device path where nothing the host derives from the whole table changes: every new row's node type is
   already populated, every value of an indexed label on a new row is already present, every new allocatable row lies inside what the key layout was chosen for
   (nodes_patch's condition), N + m - 1 fits the rank field of the key, and id order == index order does not turn false.  Every block that depends on N, its padding
   or the words of a mask row is written into a fresh block of the new size — the planes, the narrow arrays, the merged index order, every mask row — and swapped
   in at the end; the host extends its mirrors.  Otherwise the grown table goes through nodes_upsert's own code.
   Refused before anything changes — ASCHED_ERR_INVALID: no node table, m < 0, m > 0 without index / total / allocatable, an index that a resident row or another
   new row has, a taint_off or label_off that is not ascending, id_rank without id_rank_all on a table uploaded without id ranks; ASCHED_ERR_UNSUPPORTED: the table was uploaded with alloc_by_prio or node_type_override, N + m above
   2^30, whatever the rebuild would refuse (a key beyond 128 bits, more than LIT_TMAX node types on the literal path); ASCHED_ERR_DEVICE with "the handle is as it
   was" in last_error: out of device memory for the scratch and the fresh blocks (all of it is allocated first).  Any other ASCHED_ERR_DEVICE (a failed launch or
   copy) is NOT such a refusal: the handle then needs asched_nodes_upsert.
   Not this call's job: inserting rows anywhere but at the end; total, labels or index of resident rows (asched_nodes_upsert). */
int32_t ASCHED_FN(nodes_append)(asched_t*, const asched_nodes_append_rows* rows);
/* how the last nodes_append ran: out[0] rows appended, [1] 1 = the per-node blocks changed stride (the padded node count grew), [2] 1 = the rebuild path ran, [3] why:
   0 none, 1 a node type the table did not have, 2 a known node type newly populated, 3 key layout / divisor / alignment / id order, 4 a new value of an indexed label
   (reported in preference to 1 or 2), 5 the rank field of the key is too narrow; [4] N after the call, [5..7] 0.  Zeros after nodes_upsert. */
int32_t ASCHED_FN(nodes_append_stats)(asched_t*, int32_t* out /*[8]*/);

int32_t ASCHED_FN(txn_begin)(asched_t*);    /* nodeDb.Txn(true) (nodedb.go:353) */
int32_t ASCHED_FN(txn_commit)(asched_t*);
int32_t ASCHED_FN(txn_abort)(asched_t*);

/* SelectNodeForJobWithTxn (nodedb.go:538-630). pinned_node>=0 == jctx.AssignedNode set (evicted job). */
int32_t ASCHED_FN(select_node)(asched_t*, int32_t job, int32_t pinned_node, asched_pod_result* out,
                               int32_t* preempted /*cap*/, int32_t preempted_cap, int32_t* num_preempted);
/* ScheduleManyWithTxn (nodedb.go:417-462): select+bind each member inside the caller's txn. ok=0 => caller aborts. */
int32_t ASCHED_FN(schedule_many)(asched_t*, int32_t n, const int32_t* jobs, const int32_t* pinned_nodes /*NULL*/,
                                 asched_pod_result* out /*[n]*/, int32_t* ok,
                                 int32_t* preempted, int32_t preempted_cap, int32_t* num_preempted);
/* NumExcludedNodesByReason of `job`'s last node selection (select_node, schedule_many, gang_schedule, submit_check or a round), see asched_excluded_reason.
   Entries ascending by (kind, a, b, c, required, available).  Returns the number of entries (the first `cap` are written; 0 = the job has no failed
   selection on record: never attempted, skipped by scheduling key, or failed a constraint before any node was looked at), ASCHED_ERR_UNSUPPORTED as documented
   above or when the record was dropped (more than the configured number of failed selections since the job table / round was set up, or more dynamic reasons
   than the arena holds).  asched_set_excluded_nodes: how many failed selections are kept per round / job table (default 1024; 0 = none are recorded, and the one
   wide pass per failed selection is not run). */
int32_t ASCHED_FN(excluded_nodes)(asched_t*, int32_t job, asched_excluded_reason* out, int32_t cap);
int32_t ASCHED_FN(set_excluded_nodes)(asched_t*, int32_t max_failed_selections);
/* BindJobToNode+Upsert (nodedb.go:1046-1068), EvictJobsFromNode (:1079), UnbindJobFromNode (:1108) */
int32_t ASCHED_FN(bind)(asched_t*, int32_t job, int32_t node, int32_t priority);
int32_t ASCHED_FN(evict)(asched_t*, int32_t job, int32_t node);
int32_t ASCHED_FN(unbind)(asched_t*, int32_t job, int32_t node);
/* AddEvictedJobSchedulingContextWithTxn (nodedb.go:1209) / Reset (:299).  index in [0, m): the table holds at most one entry per
   job of the job table, and the round numbers its entries 0, 1, 2 ... in eviction order (pqs.go:589-639). */
int32_t ASCHED_FN(add_evicted)(asched_t*, int32_t index, int32_t job, int32_t node);
int32_t ASCHED_FN(reset_evicted)(asched_t*);
/* NumNodes (nodedb.go:345), TotalKubernetesResources (:349: the sum of the nodes' allocatable resources, addNodeToStats :44-55) and
   NodeTypesMatchingJob (:1118-1133): how many node types the job's static requirements admit (NodeTypeJobRequirementsMet) and how many
   nodes the other types hold (the reference keys that count by a reason string; the reasons are not modelled). */
int32_t ASCHED_FN(num_nodes)(asched_t*);
int32_t ASCHED_FN(total_resources)(asched_t*, int64_t* out /*[R]*/);
int32_t ASCHED_FN(node_types_matching_job)(asched_t*, int32_t job, int32_t* num_matching_types, int32_t* num_excluded_nodes);
/* The jobs of one queue in jobdb.SchedulingOrderCompare order (jobdb/comparison.go:49-107): jobs with an active run first, then
   priority-class priority descending, queue priority ascending, (both active: run timestamp ascending,) submit time ascending, id.
   This is the order the round takes evicted jobs of a queue in (pqs.go:589-639); returns the number of jobs of the queue. */
int32_t ASCHED_FN(scheduling_order)(asched_t*, int32_t queue, int32_t* out_jobs, int32_t cap);
/* node.AllocatableByPriority, [P][R] */
int32_t ASCHED_FN(get_alloc)(asched_t*, int32_t node, int64_t* out);
int32_t ASCHED_FN(get_scheduled_at_priority)(asched_t*, int32_t job, int32_t* out, int32_t* ok); /* nodedb.go:315 */
/* ClearAllocated (nodedb.go:1178-1199): AllocatableByPriority[p] = allocatableResources for every p on every node; the
   nodes' job bookkeeping is left as it is (DeepCopyNilKeys clones the maps, internaltypes/node.go:344-372). */
int32_t ASCHED_FN(clear_allocated)(asched_t*);
/* (The HIP backend orders nodes by a packed key sized for allocatable: unbinding, after a clear, a job that was bound before it lifts a
   bucket above allocatable and is refused with ASCHED_ERR_UNSUPPORTED when the key field overflows; the submit checker's NodeDbs hold
   no jobs, submitcheck.go:180, so the reference never does that.) */
/* A batch of submit-check units against the CURRENT NodeDb state (the submit checker's NodeDb is built without jobs and
   cleared, submitcheck.go:180-188).  Unit u = jobs unit_jobs[unit_off[u] .. unit_off[u+1]) as one gang context; each unit
   runs inside its own transaction which is aborted, so units never see each other's binds (submitcheck.go:345-349).
   unit_flags[u] & ASCHED_SUBMIT_STRIP_GANG: the individual check of getIndividualSchedulingResult (submitcheck.go:272-290).
   One device launch serves the whole batch. */
int32_t ASCHED_FN(submit_check)(asched_t*, int32_t n_units, const int32_t* unit_off /*[n_units+1]*/, const int32_t* unit_jobs,
                                const int32_t* unit_flags /*[n_units] or NULL*/, asched_submit_result* out /*[n_units]*/);
/* Measurement hook (no reference counterpart): how the last submit_check ran.  out = {units answered by the wide fit kernels (individual
   checks on a pristine NodeDb), fit-kernel passes (home rows, then one per away entry), units through the sequential control launch (a NodeDb holding jobs, gang units
   with away types or with rows off the index grid, every unit off the grid on a two-word order key), gang units answered
   one workgroup per unit on a pristine NodeDb (csrc/submit_gang.h), walks over the node set the wide / capacity / gang-unit launches made (one per launch of the fit or
   capacity kernel, one per member of a gang unit, one for the index of the literal first fit: what a roofline prices), literal units: the wide units with a
   home or away mask row on the literal iteration path (a request off the index grid, several node types off it), whose rows the literal batched first fit answered
   (csrc/kernels_fit_lit.h) — counted in out[0] too}. */
int32_t ASCHED_FN(submit_stats)(asched_t*, int32_t* out /*[6]*/);
/* NodeTypesIterator order (nodeiteration.go:74-149) for req at a priority over node types `types` (node_type_override ids; ntypes<0: all types).
   Test hook for the golden orderings of nodeiteration_test.go; the HIP backend materialises its literal iterator restatement (the one rounds use
   off the index grid) in the auxiliary kernel. */
int32_t ASCHED_FN(iterate_nodes)(asched_t*, const int64_t* type_ids, int32_t ntypes, int32_t priority,
                                 const int64_t* indexed_req /*[K]*/, int32_t* out_nodes, int32_t cap, int32_t* n_out);
/* First feasible node per job at `priority` against the CURRENT state, no binding: n independent
   selectNodeForPodAtPriority calls (nodedb.go:840-879) — BASELINE config 2 ("nodedb fit kernel").  Jobs whose iteration order is the packed-key order share
   one pass over the node planes; jobs off the index grid (an unaligned request, several node types with unaligned allocatable) are answered by the literal
   iterators over an index of the level built for the call, one wavefront per distinct shape (csrc/kernels_fit_lit.h); a batch that mixes both is answered whole.
   ASCHED_ERR_UNSUPPORTED only for a job off the grid on a handle whose order key takes two words (select_node answers those). */
int32_t ASCHED_FN(fit_select_batch)(asched_t*, int32_t n, const int32_t* jobs, int32_t priority, int32_t* out_node);

/* ------------------------------------------------------------------ one pool on several GPUs (no reference counterpart: SURVEY 8e)
 * The words the collectives reduce are produced and consumed ON THE DEVICE.  A pointer marked "device-accessible" may be memory of the
 * handle's GPU — e.g. a torch tensor's data_ptr(): the caller runs ncclAllReduce / torch.distributed.all_reduce on that tensor in place
 * (RCCL over xGMI) — or ordinary host memory (the CPU tests, gloo). */
#define ASCHED_NO_NODE_WORD INT64_MAX
/* Node-partitioned exact first fit: rows [lo, hi) of the pool's nodes live in this handle.  fit_select_batch_global answers
   fit_select_batch and packs, per query, the winning node's ORDER KEY in a layout every shard shares — (floor(allocatable / resolution) on
   the indexed resources ..., rank of the node's index among ALL nodes of the pool): RoundedNodeIndexKeyFromResourceList (encoding.go:37-54)
   as one integer — so that all-reduce MIN over the shards IS the reference's "first node in index order that fits"
   (nodeiteration.go:318-382 across the shards).  No node in this shard: ASCHED_NO_NODE_WORD.  The library's own packed key is sized per
   handle; the field widths here come from the caller (the GLOBAL maxima), n_fields must equal the number of indexed resources and
   sum(field_bits) + rank_bits <= 62. */
typedef struct asched_global_key_layout {
  int32_t n_fields;
  int32_t field_bits[6];
  int32_t rank_bits;
  const int32_t* global_rank;   /* [N] rank of each local node's index among all nodes of the pool; NULL: rank_offset + the local rank */
  int64_t rank_offset;
} asched_global_key_layout;
int32_t ASCHED_FN(fit_select_batch_global)(asched_t*, int32_t n, const int32_t* jobs, int32_t priority, const asched_global_key_layout* layout,
                                           int64_t* out_words /* device-accessible [n] */);
/* The north_star's queue-hash round: queues are split over the ranks, every rank runs schedule_round on a full replica with the queued
   jobs of ITS queues, then ONE all-reduce SUM of the buffer round_delta fills:
     buf[node * R + r]   resources this rank's NEWLY scheduled jobs (not running before the round) committed on the node
     buf[N * R + job]    (node + 1) | (priority level << 28) if this rank newly scheduled the job (at most one rank does: it owns the job's
                         queue), plus 1 << 32 if this rank preempted the job
   round_delta_resolve reads the reduced buffer: a node whose summed commitments exceed what is free there once every rank's preemptions are
   applied is a CONFLICT; new jobs on conflict nodes (and every member of a gang that has one) are not accepted — the caller replays them in
   global order through the ordinary queue scheduler (schedule_queues) on the accepted state.  Outputs, per job: the node it runs on after
   the accepted placements and all preemptions (-1: none), the priority it is bound at there, replay flag. */
typedef struct asched_delta_summary { int32_t conflict_nodes, accepted, replay, preempted; } asched_delta_summary;
int32_t ASCHED_FN(round_delta_words)(asched_t*, int64_t* n_words);
int32_t ASCHED_FN(round_delta)(asched_t*, int64_t* buf /* device-accessible [N*R + M] */);
int32_t ASCHED_FN(round_delta_resolve)(asched_t*, const int64_t* reduced /* device-accessible */, asched_delta_summary* summary,
                                       int32_t* job_node /*[M]*/, int32_t* job_priority /*[M]*/, uint8_t* job_replay /*[M]*/);

/* ---- The communicator: RCCL over xGMI inside the library (round 4).  One communicator per handle; every collective below is enqueued on the
   HANDLE'S OWN STREAM, behind the kernels that produce the words and in front of the kernels that consume them, so there is nothing for the
   caller to order (the pointer-taking entry points above leave the collective, and the stream ordering around it, to the caller).
   No reference counterpart: FairSchedulingAlgo schedules one pool on one goroutine (scheduling_algo.go:165); this is BASELINE north_star's
   "single RCCL all-reduce over xGMI".
     asched_comm_unique_id     ncclGetUniqueId: one rank creates it, the caller's control plane (the Go scheduler's leader election / gRPC, an MPI
                               broadcast, a file) hands the 128 bytes to every rank
     asched_comm_init          ncclCommInitRank on the handle's GPU; blocks until all `world` ranks have called it
     asched_comm_init_external any other transport (MPI, gloo in the CPU tests of this repository): the library calls `fn` with its stream idle;
                               `buf` is memory of the handle's GPU in the HIP library (host memory in the CPU build of the tests), count int64 words
     asched_comm_destroy       also done by asched_destroy
   op: 0 SUM, 1 MIN, 2 MAX (int64). */
typedef struct asched_unique_id { char bytes[128]; } asched_unique_id;
typedef int32_t (*asched_allreduce_fn)(void* ctx, void* buf, int64_t count, int32_t op);
int32_t ASCHED_FN(comm_unique_id)(asched_unique_id* out);
int32_t ASCHED_FN(comm_init)(asched_t*, const asched_unique_id* id, int32_t rank, int32_t world);
int32_t ASCHED_FN(comm_init_external)(asched_t*, asched_allreduce_fn fn, void* ctx, int32_t rank, int32_t world);
int32_t ASCHED_FN(comm_destroy)(asched_t*);
int32_t ASCHED_FN(comm_rank)(asched_t*, int32_t* rank, int32_t* world);   /* world = 1 without a communicator */
/* EXACT, node-partitioned: fit_select_batch over a pool whose node rows are split across the ranks of the communicator — k_fit_batch over this
   rank's rows, the order-key words packed on the device (fit_select_batch_global), ONE all-reduce MIN on the handle's stream, the winners unpacked:
   out_rank[i] = rank of the chosen node's index among ALL nodes of the pool (layout->rank_offset + local rank, or layout->global_rank), -1 none.
   Every rank must call it with the same jobs / priority / layout widths.  MIN over the shards IS the reference's first node in index order
   that fits (nodedb.go:840-879, nodeiteration.go:318-382). */
int32_t ASCHED_FN(fit_select_batch_sharded)(asched_t*, int32_t n, const int32_t* jobs, int32_t priority, const asched_global_key_layout* layout,
                                            int32_t* out_rank /*[n]*/);
/* EXACT, ONE pool's round on several GPUs (SURVEY 8e "Nodes (exact)"): every rank of the communicator holds the WHOLE pool (same nodes, jobs, queues: the state of a
   round is tens of megabytes) and runs the whole round, but after shard_round(h, 1) the round's wide passes over the nodes — the first-fit plane scan and the per-node
   evaluation of fair-share preemption (selectNodeForPodAtPriority nodedb.go:840-928, selectNodeForJobWithFairPreemption :935-1043) — look at this rank's 1/world of the
   node words only, and every pass ends with ONE all-reduce MIN of two 64-bit words (the minimum order key; the complement of the maximum evicted-table index) on the
   handle's communicator: RCCL on a side stream while the round kernel waits, or the external transport, which is then called with ASCHED_ALLREDUCE_HOST_WORDS or-ed into
   `op` (buf is host memory: reduce it in place, do not synchronise the device — the round kernel is running).  The minimum over the shares IS the unsharded pass's answer,
   so every rank computes the reference's round, bit for bit the same one.  Every rank must run the same calls on the same inputs.  shard_exchanges: all-reduces of the
   handle's last round (of its last control launch outside a round); with the GPU-to-GPU exchange below: as the round kernel counted them.  Not measured on more than one GPU. */
#define ASCHED_ALLREDUCE_HOST_WORDS 16
int32_t ASCHED_FN(shard_round)(asched_t*, int32_t on);
int64_t ASCHED_FN(shard_exchanges)(asched_t*);
/* The same exchange GPU-to-GPU, without the host (and without a communicator): every replica owns an exchange area in its HBM; the control wave of its round kernel stores
   its two words into its slot of EVERY replica's area (over xGMI for a remote one) and watches its own area fill.  shard_area: this handle's area — its device pointer and
   the hipIpcMemHandle_t bytes (all zero where the runtime cannot export it) for replicas in other processes, who map it with shard_open.  shard_peers(areas[world], world,
   rank): areas[r] = replica r's area as THIS process addresses it (areas[rank] = the own one); switches the handle's rounds to sharded passes with the direct exchange;
   world <= 64.  shard_peers(NULL, ..) switches back to whole passes.  Order: every replica calls shard_area (allocates + zeroes), the caller distributes the pointers /
   handles (that is also the barrier the zeroing needs), every replica calls shard_peers, then the replicas run the same rounds.  A replica that leaves a round early
   (deadline) leaves the counters out of step: start over with fresh handles.  Exercised with two replicas on ONE GPU (two round kernels side by side); never over xGMI. */
typedef struct asched_shard_area_t { void* ptr; char ipc[64]; } asched_shard_area_t;
int32_t ASCHED_FN(shard_area)(asched_t*, asched_shard_area_t* out);
int32_t ASCHED_FN(shard_open)(asched_t*, const char* ipc /*[64]*/, void** out);
int32_t ASCHED_FN(shard_peers)(asched_t*, void* const* areas /*[world]*/, int32_t world, int32_t rank);
/* APPROXIMATE (labelled so everywhere), queue-hash round: round_delta + ONE all-reduce SUM + round_delta_resolve as one stream-ordered sequence
   on the handle's stream; outputs as round_delta_resolve. */
int32_t ASCHED_FN(round_exchange)(asched_t*, asched_delta_summary* summary, int32_t* job_node /*[M]*/, int32_t* job_priority /*[M]*/, uint8_t* job_replay /*[M]*/);

/* ------------------------------------------------------------------ float helpers (goldens) */
/* DominantResourceFairness.UnweightedCostFromAllocation (fairness/fairness.go:103-105) */
double ASCHED_FN(drf_cost)(asched_t*, const int64_t* alloc /*[R]*/, const int64_t* total /*[R]*/);
/* SchedulingContext.updateFairShares (context/scheduling.go:262-342). cds = constrainedDemandShare per queue. */
int32_t ASCHED_FN(fair_shares)(asched_t*, int32_t q, const int32_t* name_rank, const double* weight, const double* cds,
                               double* fair_share, double* demand_capped, double* uncapped);

/* QueueCandidateGangIteratorPQ ordering (queue_scheduler.go:738-798): out_order = the item indices as sort.Sort leaves them
   (queue_scheduler_test.go:995-1164 drive Less exactly this way).  n <= 64.  Cross-pool "away" items do not exist within one pool.
   packed_agrees (may be NULL): 1 when, for every pair of items, the lexicographic key the fast path orders queues by (DESIGN 3.1
   item 4) gives the same verdict as Less; the CPU oracle reports 1. */
typedef struct asched_pq_item {
  double proposed_cost, current_cost, budget, item_size;   /* proposedQueueCost, currentQueueCost, queueBudget, itemSize */
  int32_t pc_priority, scheduling_priority, name_rank, away; /* priorityClassPriority, schedulingPriority, rank of the queue name, item.away (a cross-pool job's queue context) */
} asched_pq_item;
/* compare_scheduling_priority: bit 0 = compareSchedulingPriority, bit 1 (ASCHED_PQ_HOME_FIRST) = preemptCrossPoolJobsFirst: home items before away items
   (queue_scheduler.go:744-746) */
#define ASCHED_PQ_HOME_FIRST 2
int32_t ASCHED_FN(pq_order)(asched_t*, int32_t n, const asched_pq_item* items, int32_t prioritise_larger_jobs, int32_t compare_scheduling_priority,
                            int32_t* out_order /*[n]*/, int32_t* packed_agrees);

/* MarketBasedCandidateGangIterator (market_iterator.go:32-295): the order in which the market-driven candidate iterator yields the queues' jobs.  Queue q
   holds jobs[off[q] .. off[q+1]) in its iterator's order; out_queue[i] = the queue of the i-th Peek (Clear after each).  The priority queue is
   container/heap over MarketIteratorPQ.Less (:228-273), which is NOT a strict weak order — its round-robin clause reads the queue and price of the
   previous result — so the heap's up / down moves are restated literally (HIP backend: armada_amd/csrc/round_market.h, run by the auxiliary kernel).
   Test hook (market_iterator_test.go:17-122).  The market-driven ROUND — evict-everything node evictor, spot price / second-price billing, indicative
   pricer — is not built yet. */
typedef struct asched_market_job {
  double price;                    /* job.GetBidPrice(pool) */
  int64_t runtime, submit_time;    /* item.runtime as updatePQItem computes it (now - LatestRun().Created() for a job that is not queued, else 0); SubmitTime */
  int32_t queued, away;            /* job.Queued(); !IsHomeJob(pool) */
} asched_market_job;
int32_t ASCHED_FN(market_iterate)(asched_t*, int32_t nq, const int32_t* name_rank /*[nq]*/, const int32_t* off /*[nq+1]*/, const asched_market_job* jobs,
                                  int32_t preempt_cross_pool_jobs_first, int32_t* out_queue /*[off[nq]]*/);

/* jobdb.MarketSchedulingOrderCompare (jobdb/comparison.go:113-170): the order of a queue's jobs under market-driven scheduling — priority class priority
   (higher first), bid price for the pool (higher first), a job with an active run before one without, older run first, earlier submit time, job id.
   *out_sign = -1 / 0 / +1.  Test hook like market_iterate (comparison_test.go:76-178). */
typedef struct asched_market_cmp_job {
  double bid_price;                              /* job.GetBidPrice(currentPool) */
  int64_t active_run_timestamp, submit_time;
  int32_t pc_priority, active, id_rank, pad_;   /* priorityClass.Priority; activeRun != nil && !InTerminalState(); rank of the job id (equal rank = same id) */
} asched_market_cmp_job;
int32_t ASCHED_FN(market_compare)(asched_t*, const asched_market_cmp_job* a, const asched_market_cmp_job* b, int32_t* out_sign);
/* MarketDrivenMultiJobsIterator (jobiteration.go:232-321) over two InMemoryJobIterators (:22-65): the merge of a queue's two job lists by
   MarketSchedulingOrderCompare, with OnlyYieldEvicted called before the (only_evicted_after + 1)-th Next (negative: never).  out = the yielded jobs, list 1
   as its index, list 2 as n1 + index.  Test hook (jobiteration_test.go:150-232). */
int32_t ASCHED_FN(market_multi_iterate)(asched_t*, int32_t n1, const asched_market_cmp_job* list1, const uint8_t* evicted1, int32_t n2,
                                        const asched_market_cmp_job* list2, const uint8_t* evicted2, int32_t only_evicted_after, int32_t* out, int32_t* n_out);

/* ------------------------------------------------------------------ round level */
/* Builds round state: ConstructNodeDb/populateNodeDb (bind every running job, scheduling_algo.go:738-781,
   1019-1098) + constructSchedulingContext + UpdateFairShares (:783-867).  Untimed "input build". */
int32_t ASCHED_FN(round_prepare)(asched_t*, const asched_queues* queues);
/* round_prepare with the queued lists derived on the device from the resident job order — what NewQueuedJobsIterator does when it reads
   repo.QueuedJobs(queue, pool, sortOrder), a view of the resident jobDb and not a list handed in per cycle (scheduling/jobiteration.go:144-160; the host-side walk it
   replaces is queuedJobs of integration/gpu_round.go Schedule).  queues->queued_off and queues->queued_jobs must be NULL; every other field means what it means to
   round_prepare.  The list of queue q < queues->q is every row with queue == q that has no run and is not named in `held`, in the resident order (per queue the
   SchedulingOrderCompare order jobs_set built and jobs_patch / jobs_append / jobs_delete keep exact); rows of queues >= queues->q take no part.  `held` is per call and
   nothing of it is stored: it carries what the reference's per-pool queued view leaves out (a queued job whose pools exclude this pool, a row the host keeps but does
   not want scheduled this cycle).  Duplicates are allowed; a held row that has a run has no effect.  Costs O(n_held) per call on top of one pass over the job table.
   Refused before anything on the handle changes — ASCHED_ERR_INVALID: non-NULL queued_off or queued_jobs, n_held < 0, n_held > 0 without held, a held id outside
   [0, M), nodes or jobs not set; ASCHED_ERR_UNSUPPORTED: more than 4096 queues, a job set that carries the market order (uploaded with bid prices or after
   asched_set_market — the market order is another order than the resident one: give round_prepare the lists in that order). */
int32_t ASCHED_FN(round_prepare_resident)(asched_t*, const asched_queues* queues,
                                          int32_t n_held, const int32_t* held /*[n_held] rows left out of this round's queued lists, or NULL*/);
/* The queued lists the last round_prepare or round_prepare_resident left on the device, i.e. what the round walks (the jobs NewQueuedJobsIterator yields per queue,
   jobiteration.go:162-176).  Writes off[0..Q]; writes jobs[0..total) only if cap >= total.  Returns the total length, or ASCHED_ERR_INVALID before any prepare. */
int32_t ASCHED_FN(round_queued)(asched_t*, int32_t* off /*[Q+1]*/, int32_t* jobs /*[cap]*/, int32_t cap);
/* PreemptingQueueScheduler.Schedule (preempting_queue_scheduler.go:86-289) — what the metric times.
   Result buffers are owned by the handle until the next round_prepare/destroy. */
int32_t ASCHED_FN(schedule_round)(asched_t*, asched_round_result* out);

/* QueueScheduler.Schedule (queue_scheduler.go:94-304) over the queued jobs only — no eviction phases; the entry the
   reference's queue_scheduler_test.go drives.  `preempted_*` lists the fair-share victims (sctx.PreemptedJobIds).
   On a market-driven pool (set_market) the queue is picked by the market iterator and the spot price is set, as NewQueueScheduler
   does when marketDriven is true (queue_scheduler.go:73-74, 176-203). */
int32_t ASCHED_FN(schedule_queues)(asched_t*, asched_round_result* out);

/* ---- who preempted each job, and by which kind of preemption (PopulatePreemptionDescriptions, preemption_description.go:21-81, called at the end of
   PreemptingQueueScheduler.Schedule, preempting_queue_scheduler.go:268).  type is jctx.PreemptionType (context/pod.go:22-31; cycle_metrics.go:710-711
   counts preemptions by it), preempting_job / preempted_sibling are jctx.PreemptionDetails (PreemptingJob: nodedb.go:1034, applied at gang_scheduler.go:268-273;
   PreemptedSiblingJob: nodedb.go:514-520) — what the JobRunPreempted event carries as PreemptingJobId (scheduler.go:814,912).  No description strings cross
   the boundary: the caller formats them with the templates of preemption_description.go:11-19. */
#define ASCHED_PREEMPTION_UNKNOWN 1       /* context.Unknown (pod.go:25): not rescheduled, nothing on record, no urgency-scheduled job on its node (:50-51) */
#define ASCHED_PREEMPTION_UNKNOWN_GANG 2  /* context.UnknownGangJob (pod.go:26): the same for a gang member (:46-48) */
#define ASCHED_PREEMPTION_FAIRSHARE 3     /* context.PreemptedWithFairsharePreemption (pod.go:27): PreemptionDetails.PreemptingJob is set (:28-42); also on a market-driven pool */
#define ASCHED_PREEMPTION_URGENCY 4       /* context.PreemptedWithUrgencyPreemption (pod.go:28): caused by one of the jobs of its candidate slice (:53-62) */
#define ASCHED_PREEMPTION_OPTIMISER 5     /* context.PreemptedWithOptimiserPreemption (pod.go:29; optimiser/gang_scheduler.go:226-227) */
typedef struct asched_preemption_cause {
  int32_t type;               /* ASCHED_PREEMPTION_* */
  int32_t preempting_job;     /* FAIRSHARE, OPTIMISER: PreemptionDetails.PreemptingJob / the job the optimiser placed; otherwise -1 */
  int32_t preempted_sibling;  /* FAIRSHARE: PreemptionDetails.PreemptedSiblingJob — the directly preempted member of its gang that pulled it in; -1 = preempted directly */
  int32_t cand_off;           /* URGENCY: candidates[cand_off .. cand_off + cand_count) are the jobs scheduled with urgency preemption on its node */
  int32_t cand_count;
  int32_t pad_;
} asched_preemption_cause;
/* Causes of the last round's preempted jobs: entry i belongs to asched_round_result.preempted_job[i].  `candidates` receives the round's jobs with method
   ASCHED_METHOD_URGENCY grouped by node (calculateJobsScheduledWithUrgencyBasedPreemptionByNode :67-81), each once, ascending job index within a node (the
   reference's order is that of a slice built while ranging over a map of scheduled jobs: undefined; ascending is this ABI's rule); every preempted job of a node
   shares the node's slice.  *num_candidates: how many were written.  Valid after schedule_round and schedule_queues (there every preempted job is a fair-share
   victim), optimiser and market-driven rounds and each replica of a sharded round included; computed only when asked for (a grid-wide join over the result lists in
   HBM, csrc/kernels_preempt_join.h).  ASCHED_ERR_INVALID with no round result on the handle or after round_exchange (the approximate queue-hash mode moves
   preemptions between replicas: the per-job record no longer describes the resolved round), and when cap < num_preempted or cand_cap < the number of candidates:
   *num_candidates then holds the needed cand_cap and last_error both sizes. */
int32_t ASCHED_FN(round_preemption_causes)(asched_t*, asched_preemption_cause* out /*[cap]*/, int32_t cap, int32_t* candidates /*[cand_cap]*/, int32_t cand_cap,
                                           int32_t* num_candidates);
/* The same join on the caller's lists (PopulatePreemptionDescriptions as a function of its two arguments; test hook like asched_pq_order, for
   preemption_description_test.go:18-165).  sched_*: [ns] the scheduled jobs, their nodes (in [0, N) of the handle's nodes) and ASCHED_METHOD_*; pre_*: [np] per
   preempted job its node, PreemptingJob or -1, PreemptedSiblingJob or -1 (-2: its description is already set by the fairness optimiser, :25-27 — type OPTIMISER)
   and whether it is in a gang.  Candidates of a node come in the order of the scheduled list (a stable sort by node).  out: [np]; candidates: [cand_cap], at most ns are needed. */
int32_t ASCHED_FN(preemption_join)(asched_t*, int32_t ns, const int32_t* sched_job, const int32_t* sched_node, const int32_t* sched_method, int32_t np,
                                   const int32_t* pre_node, const int32_t* pre_by, const int32_t* pre_sibling, const uint8_t* pre_in_gang,
                                   asched_preemption_cause* out, int32_t* candidates, int32_t cand_cap, int32_t* num_candidates);
/* ---- the evictor result of a round (SchedulingInformation.EvictorResult, scheduling/result.go:81-94, filled at preempting_queue_scheduler.go:274-281): what the
   balancing evictor of phase 1 did (EvictorResult, eviction.go:27-79).  Consumers in the reference: the cycle metrics (metrics/cycle_metrics.go:629-647: evicted
   jobs and resources per queue, preemptibility per node), the async runner (runner/async.go:435) and evict's log line (preempting_queue_scheduler.go:308).
   Recorded on the device while phase 1 runs (csrc/kernels_evict_report.h) and only when switched on: nothing of it can be recovered after the round.  All values are
   as of the moment the node evictor of phase 1 runs (preempting_queue_scheduler.go:96-138).
   Reason bits of a node, numbered in the alphabetical order of the reference's reason strings, so that ascending bit order is the sorted, comma-joined string of
   makeNodePreemptiblityStats (eviction.go:275-285); no strings cross the boundary.  missing_annotations / missing_node_selector (preempting_queue_scheduler.go:109-116)
   have no counterpart behind this boundary. */
#define ASCHED_EVR_ALL_JOBS_PREEMPTIBLE 1        /* "all_jobs_preemptible" (eviction.go:234): the node has jobs and no reason is set; alone */
#define ASCHED_EVR_BELOW_PROTECTED_FAIR_SHARE 2  /* "below_protected_fair_share" (preempting_queue_scheduler.go:131-133) */
#define ASCHED_EVR_INVALID_QUEUE 4               /* "invalid_queue" (:105-108): a job whose queue is outside [0, Q) */
#define ASCHED_EVR_JOB_NOT_PREEMPTIBLE 8         /* "job_not_preemptible" (:120-122) */
#define ASCHED_EVR_NODE_EMPTY 16                 /* "node_empty" (eviction.go:89-96): no job holds resources on the node */
#define ASCHED_EVR_NODE_UNSCHEDULABLE 32         /* "node_unschedulable" (eviction.go:203-206, 228-230) */
typedef struct asched_evictor_report {
  int32_t num_nodes, num_queues, num_resources, num_evicted;
  int32_t num_affected_nodes, pad_;            /* len(AffectedNodesById) */
  const uint8_t* node_preemptible;             /* [N] NodePreemptiblityStats.Preemptible */
  const uint8_t* node_reasons;                 /* [N] ASCHED_EVR_* bits */
  const int32_t* node_evicted_jobs;            /* [N] jobs evicted from the node (>0 = affected) */
  const int32_t* queue_evicted_jobs;           /* [Q] EvictorPerQueueStats.EvictedJobCount (eviction.go:60-71) */
  const int64_t* queue_evicted_resources;      /* [Q][R] EvictedResources: the sum of KubernetesResourceRequirements — the request rows with the floating columns as 0 */
  const int32_t* queue_evicted_off;            /* [Q+1] into the two lists below */
  const int32_t* evicted_job;                  /* [num_evicted] grouped by queue, SchedulingOrderCompare order inside a queue (the phase-1 evList) */
  const int32_t* evicted_node;                 /* [num_evicted] NodeIdByJobId */
} asched_evictor_report;
/* The switch, off by default.  Off, schedule_round issues exactly the launches it issues without the feature and allocates nothing for it.  On, a round that goes
   through the split launch sequence (one- and two-word-key handles, optimiser rounds, asched_shard_round) queues three more launches in phase 1 — a pass over the
   jobs, one over the nodes, one over the compacted evicted list — and waits for none of them.  The evicted set is EvictedJctxsByJobId after evictGangs has been
   merged in (preempting_queue_scheduler.go:316-326); the gang evictor's own node stats are discarded, as in the reference. */
int32_t ASCHED_FN(set_evictor_report)(asched_t*, int32_t on);
/* The report of the last schedule_round.  The buffers belong to the handle until the next round_prepare, like the round result.  ASCHED_ERR_INVALID: the switch is
   off, no round has completed since it was turned on, or the last round failed or timed out.  ASCHED_ERR_UNSUPPORTED (last_error names the cause): a market-driven
   handle (set_market: the whole round is one launch of the auxiliary kernel), ASCHED_SINGLE_LAUNCH=1, and after round_exchange (the queue-hash mode moves
   preemptions between replicas: the record describes this replica's own round). */
int32_t ASCHED_FN(round_evictor_report)(asched_t*, asched_evictor_report* out);
/* GangScheduler.Schedule (gang_scheduler.go:100-148) for one gang of queued jobs against the current round state. */
int32_t ASCHED_FN(gang_schedule)(asched_t*, int32_t n, const int32_t* jobs, int32_t* ok, int32_t* reason, asched_pod_result* out /*[n]*/);
/* sctx counters: out = {NumScheduledJobs, NumScheduledGangs, NumEvictedJobs, len(UnfeasibleSchedulingKeys)} (context/scheduling.go:55-69) */
int32_t ASCHED_FN(round_counters)(asched_t*, int32_t* out /*[4]*/);
/* Measurement hook (no reference counterpart): device time of the kernels behind the last call, taken with HIP events
   on the stream the kernels were launched on.  out[0] = ms of the last schedule_round/schedule_queues device work,
   out[1] = ms of the last fit_select_batch (or optimiser k_opt_score) kernel, or of the kernels of the last round_preemption_causes / preemption_join if that came later, out[2] = kernel launches behind out[0], out[3] = ms of the last submit_check launch.
   The CPU oracle reports zeros. */
int32_t ASCHED_FN(kernel_times)(asched_t*, double* out /*[4]*/);
/* Measurement hook (no reference counterpart): where the device time of the last schedule_round went.  out = {whole launch sequence ms (HIP
   events on the stream), ms inside the persistent k_control launches (the two sequential passes), kernel launches, host ms of the grid-wide
   evict-1 / evict-3 / final phases including their count read-backs, 0, 0}.  The CPU oracle reports zeros. */
int32_t ASCHED_FN(round_timing)(asched_t*, double* out /*[8]*/);
/* Measurement hook (no reference counterpart): how the last round ran on the device.  out = {fast iterations, generic
   iterations, base scan steps, window refills, max live dirty nodes (L0), fast replay steps, L0 overflows,
   fast structure active at the end, [8..15] kilo-ticks per phase, [16..19] stream runs / entries bound in them / stream entries prepared / emitted,
   [20] iterations whose job needed preemption and stayed in the fast loop, [21] picks the split node engine's short path took
   (device only: the CPU build leaves it 0; ASCHED_HC_SHORT=0 turns the path off), [22] gangs placed nested inside stream runs (the CPU build of the tests only: the device
   leaves it 0), [23] streams the bulk merge turned away for their length (the CPU build of the tests only), [24] picks the split node engine's clean short path took
   (device only, like [21], and switched off with it)}.  The CPU oracle reports zeros. */
int32_t ASCHED_FN(round_stats)(asched_t*, int32_t* out /*[25]*/);
/* Hard timeout of a round (maxSchedulingDuration, config/scheduler/config.yaml:83; scheduling_algo.go:130-134 wraps the context in
   WithTimeout, queue_scheduler.go:105-112 checks ctx.Done() every loop iteration and returns ctx.Err()).  asched_set_deadline: every
   following schedule_round / schedule_queues is cancelled `seconds` after it starts (0 = none).  asched_cancel = the context's cancel
   function: callable from ANY thread while a round is in flight; between rounds it hits the next one ("context already done").  A
   cancelled round returns ASCHED_ERR_TIMEOUT, delivers no result (scheduling_algo.go:262-270 applies nothing on error) and leaves the
   handle unprepared: round_prepare builds the next round from scratch. */
int32_t ASCHED_FN(set_deadline)(asched_t*, double seconds);
int32_t ASCHED_FN(cancel)(asched_t*);
/* Withdraws a cancel request that no round has consumed yet — for a caller whose watcher thread fired asched_cancel a moment after the round it was
   meant for had returned (the request would otherwise hit the NEXT round on this handle).  Same thread as the round calls; never during a round. */
int32_t ASCHED_FN(cancel_clear)(asched_t*);
/* IndexedNodeLabelValues (nodedb.go:340-343): values of an indexed node label present on the nodes (ascending interned id).
   Returns their number, or -1 when the label is not indexed (ok == false). */
int32_t ASCHED_FN(indexed_node_label_values)(asched_t*, int32_t label_key, int32_t* out_values, int32_t cap);
/* GetNode / GetNodeWithTxn (nodedb.go:358-394), the mutable part of *Node: jobs holding resources on the node (AllocatedByJobId), their
   evicted flag (EvictedJobRunIds) and scheduled-at priority; any out pointer may be NULL.  Returns the number of jobs on the node. */
int32_t ASCHED_FN(get_node_jobs)(asched_t*, int32_t node, int32_t* out_jobs, uint8_t* out_evicted, int32_t* out_priority, int32_t cap);
/* GetNodes / GetNodesWithTxn (nodedb.go:396-415): AllocatableByPriority of n nodes ([n][P][R]) in one download; nodes == NULL: all n == NumNodes nodes */
int32_t ASCHED_FN(get_nodes_alloc)(asched_t*, int32_t n, const int32_t* nodes, int64_t* out);
/* Upsert / UpsertWithTxn of one node (nodedb.go:1154-1175): replaces the node's AllocatableByPriority ([P][R]) and rebuilds its order key
   at every priority.  Job bookkeeping travels through bind / evict / unbind. */
int32_t ASCHED_FN(node_upsert)(asched_t*, int32_t node, const int64_t* alloc_by_prio);

/* ------------------------------------------------------------------ experimental fairness optimiser (scheduling/optimiser)
 * One job against EVERY node: PreemptingNodeScheduler.Schedule (optimiser/node_scheduler.go:42-132) per node — static requirements, fit at
 * the evicted priority, else the node's preemptible non-gang jobs scheduled at a priority <= the job's, ordered per queue (scheduled-at
 * priority, cost, age, id; preemption_info.go:23-55) and globally (priority preemptions first, then the queue whose cost after the
 * preemption stays highest; :57-91), preempted one at a time until the job fits; schedulingCost = DRF cost of the victims that bring their
 * queue to or below its fair share (:203-232), maximumQueueImpact = largest |cost change| / current cost over the queues (:101-113) — and
 * the candidate selection of FairnessOptimisingGangScheduler.scheduleOnNodes for that job (gang_scheduler.go:100-141): nodes in id order,
 * the first node that needs no preemption wins outright, otherwise nodes whose fairness improvement (cost of the job / scheduling cost,
 * in percent minus 100) exceeds the threshold, ordered by (schedulingCost, maximumQueueImpact) (scheduling_result.go:49-68).  The reference
 * breaks remaining ties by a random ULID; here the node with the smaller id rank wins.  Queue costs / fair shares / weights are the round
 * state of the handle (round_prepare, or whatever rounds ran since).  Nothing is applied: the caller unbinds the victims and binds the job
 * (markJobsScheduledAndPreempted, :173-246) through asched_unbind / asched_bind.
 * max_job_size_to_preempt: [R] or NULL, 0 = no limit on that resource (node_scheduler.go:248-268).  now_ms: the clock the job ages are taken
 * from (age = now - asched_jobs.run_timestamp / 1e6; jobs scheduled in this round have age 0).
 * per_node (optional, [NumNodes]): every node's result, for callers that schedule gangs member by member. */
typedef struct asched_opt_result {
  int32_t node;                  /* -1 = no candidate */
  int32_t num_preempted;         /* len(jobIdsToPreempt) of the chosen node */
  double scheduling_cost;
  double maximum_queue_impact;
} asched_opt_result;
typedef struct asched_opt_node_score { int32_t scheduled; int32_t num_preempted; double scheduling_cost; double maximum_queue_impact; } asched_opt_node_score;
int32_t ASCHED_FN(optimiser_schedule_job)(asched_t*, int32_t job, double min_fairness_improvement_pct, const int64_t* max_job_size_to_preempt,
                                          int64_t now_ms, asched_opt_result* out, int32_t* preempted /*cap*/, int32_t preempted_cap,
                                          asched_opt_node_score* per_node);

/* The experimental fairness optimiser as part of the round (preempting_queue_scheduler.go:224-253, 666-710): after the second pass
   OptimisingQueueScheduler.Schedule (optimising_queue_scheduler.go:58-180) walks the queued gangs of the queues that are below their fair share in cost
   order, and FairnessOptimisingGangScheduler.Schedule (optimiser/gang_scheduler.go:45-254) places each one by scoring EVERY node (asched_optimiser_schedule_job's
   kernel), preempting the cheapest set of running jobs; its scheduled / preempted jobs are merged into the round's result (method ASCHED_METHOD_OPTIMISER).
   configuration.OptimiserConfig (configuration.go:517-537); NULL or enabled == 0: off (the default).  Applies to the following schedule_round calls.
   Node-uniformity groups are tried in ascending interned label value and remaining ties go to the earlier node id (the reference draws random ULIDs). */
typedef struct asched_optimiser_config {
  uint8_t enabled; uint8_t pad_[7];
  double min_fairness_improvement_pct;             /* MinimumFairnessImprovementPercentage */
  int32_t max_jobs_per_round; int32_t pad2_;       /* MaximumJobsPerRound */
  const int64_t* max_job_size_to_preempt;          /* [R] or NULL; 0 = no limit on that resource (node_scheduler.go:248-268) */
  const int64_t* min_job_size_to_schedule;         /* [R] or NULL */
  const double* max_resource_fraction_to_schedule; /* [R] or NULL = +Inf everywhere (MaximumResourceFractionToSchedule) */
  int64_t now_ms;                                  /* the clock job ages are taken from (asched_optimiser_schedule_job) */
} asched_optimiser_config;
int32_t ASCHED_FN(set_optimiser)(asched_t*, const asched_optimiser_config* cfg);

/* Market-driven scheduling of a pool (configuration.MarketSchedulingConfig; preempting_queue_scheduler.go:61-62): the following schedule_round calls
     - let the node evictor take EVERY job of the pool (pqs.go:117-119; cross-pool away jobs excepted, :102-104) — the prices decide who comes back;
     - order each queue's evicted jobs with jobdb.MarketSchedulingOrderCompare (pqs.go:292-295, jobdb/comparison.go:113-170) and merge them with the queued jobs by the
       same comparer (MarketDrivenMultiJobsIterator, jobiteration.go:232-321; the caller passes asched_queues.queued_jobs in that order: jobdb.PriceOrder);
     - pick the next queue with MarketBasedCandidateGangIterator (market_iterator.go: bid price, running before queued, round robin between queues at the same price ...),
       a literal container/heap because its Less reads the previous result; the queues are pushed in queue-index order (the reference ranges over a Go map);
     - set the spot price to the lowest bid of the gang that takes the DRF cost of what this pass has scheduled beyond spot_price_cutoff, mark what is in the queue
       contexts at that moment billable, and bill the price-setting queue the highest competing bid (queue_scheduler.go:177-203);
     - do not run the fairness optimiser (pqs.go:224).
   A fair-share preemption rate limiter together with market-driven scheduling is ASCHED_ERR_INVALID (the reference rejects it at config validation).  The runtime the
   reference compares between two running jobs (time.Now() - run.Created) orders like -run_timestamp: no clock is read.  NULL or enabled == 0: off (the default). */
typedef struct asched_market_config { uint8_t enabled; uint8_t pad_[7]; double spot_price_cutoff; } asched_market_config;
int32_t ASCHED_FN(set_market)(asched_t*, const asched_market_config* cfg);
/* What the last market-driven round left in the scheduling context: sctx.SpotPrice (has_spot_price 0: nil), per queue qctx.GetBillableResource() (floored at zero) and
   qctx.BillablePriceOverride (context/queue.go:39-44, 108-127).  Buffers are owned by the handle until the next round. */
typedef struct asched_market_outcome {
  int32_t has_spot_price; int32_t pad_;
  double spot_price;
  const int64_t* queue_billable_resource;      /* [q][R] */
  const double* queue_billable_price_override; /* [q] */
  const uint8_t* queue_has_price_override;     /* [q] */
} asched_market_outcome;
int32_t ASCHED_FN(market_result)(asched_t*, asched_market_outcome* out);

/* The indicative gang pricer of a market-driven pool (scheduling/pricer/gang_pricer.go:48-161, node_scheduler.go:41-146; called after the round by
   MarketDrivenIndicativePricer.Price, preempting_queue_scheduler.go:248-252, 641-664): the lowest price at which a gang could be scheduled on the NodeDb as it stands.
   Per member, in order, MinPriceNodeScheduler.Schedule scores EVERY node of the uniformity group (one wide pass, k_price_score): static requirements, fit at the
   evicted priority (price 0), else ALL jobs on the node except the gang's own members — whatever their priority class or preemptibility — ordered by (bid price,
   age, id) and preempted one at a time until the member fits: price = the last victim's bid.  The node with the lowest price takes the member (the first price-0
   node in id order wins outright; the reference breaks other ties by a random ULID, here the earlier node id), its victims are unbound and the member is bound
   (on a transaction that is aborted at the end: no side effects), and the gang's price is the highest member price; over the uniformity groups (label values in
   ascending interned order) the cheapest schedulable group wins.  `jobs` are rows of the job set (the synthetic jobs of a configuration.GangDefinition are uploaded
   like any other job, queued nowhere); bids are asched_jobs.bid_price; ages are now_ms minus the lease time.
   reason: 0, ASCHED_REASON_JOB_DOES_NOT_FIT / ASCHED_REASON_GANG_DOES_NOT_FIT, or one of the two below. */
#define ASCHED_PRICE_REASON_LABEL_NOT_INDEXED 101   /* "uniformity label is not indexed" (gang_pricer.go:18) */
#define ASCHED_PRICE_REASON_NO_NODES_WITH_LABEL 102 /* "no nodes with uniformity label" (:19) */
typedef struct asched_gang_price { int32_t evaluated, schedulable; double price; int32_t reason, pad_; } asched_gang_price;
int32_t ASCHED_FN(price_gang)(asched_t*, int32_t n, const int32_t* jobs, int64_t now_ms, asched_gang_price* out);
/* MinPriceNodeScheduler.Schedule (node_scheduler.go:41-107) for one job against every node (test hook for node_scheduler_test.go and the differential tests):
   per node scheduled / price / number of victims; for `detail_node` >= 0 also its victims in preemption order. */
typedef struct asched_price_node_score { int32_t scheduled, num_preempted; double price; } asched_price_node_score;
int32_t ASCHED_FN(price_job_on_nodes)(asched_t*, int32_t job, int64_t now_ms, asched_price_node_score* per_node /*[N]*/, int32_t detail_node,
                                      int32_t* preempted /*[cap]*/, int32_t cap);

/* 1 if the job's scheduling key is registered in sctx.UnfeasibleSchedulingKeys (gang_scheduler.go:80-95) */
int32_t ASCHED_FN(job_key_unfeasible)(asched_t*, int32_t job, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ARMADA_SCHED_H */
