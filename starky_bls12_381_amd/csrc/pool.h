// A proof pool's job and the rules that say which queued job goes next (pool.cpp) -- plain functions over plain inputs, apart from the
// threads that apply them under the pool's lock, so that a test can call them -- and what a multi-device handle (multipool.cpp) reads
// from a pool to place work.
#pragma once
#include <deque>
#include <map>
#include <vector>

#include "airs.h"
#include "trace_input.h"

namespace starkhip {

enum JobKind { JOB_RECORD, JOB_PROVE, JOB_VERIFY };  // a witness job that still needs its recording; a job with its trace; a proof to check
enum class JobState { Queued, Running, Verifying, Done };  // Queued: for its recording or for a context

struct Job {
    uint64_t id = 0;
    int air = 0;
    starkhip_config_t cfg;
    JobKind kind = JOB_PROVE;
    TraceInput in;  // JOB_PROVE: the trace, in the caller's memory or in this job's own (columns, own_log, own_rows)
    const uint64_t* pis = nullptr;
    size_t n_pis = 0;
    uint64_t pow = 0;
    std::vector<const uint64_t*> columns;  // a column table's pointers (the table is copied at submit, the columns are not)
    std::vector<uint32_t> operands;   // witness jobs
    void* own_log = nullptr;          // witness jobs: the recording, freed when proven
    std::vector<uint64_t> own_pis, own_rows;  // own_rows: the toy AIR's generator writes plain rows (it does not record)
    bool big = false;
    double cost = 0;  // relative proving cost (air_cost): what the job adds to its pool's load until it is done
    bool verify = false;  // "verify_proofs" was on when it was submitted: the pool's verifier checks the proof before wait returns it
    bool check = false;   // "check_traces" was on when it was submitted: its context checks the trace against the AIR before the LDE ...
    bool fill = false;    // "fill_lookups" was on when it was submitted: its context fills the permuted columns of the AIR's lookups first
    bool fill_freq = false;  // "fill_frequencies" was on when it was submitted: its context fills the frequencies columns of the AIR's LogUp lookups first
    size_t check_list = 16;  // ... and a refusal's check blob lists this many violations ("check_trace_list" at submit)
    int hasher = 0;       // "hasher" at submit.  A Keccak job's trace commitment is its context's own launch: it is not announced to the
                          // commitment scheduler and does not move the scheduler's counters
    // result
    JobState state = JobState::Queued;
    int rc = STARKHIP_OK;
    uint64_t* proof = nullptr;
    size_t words = 0;
    // what starkhip_pool_wait reports, filled in where each value arises (times in seconds since the pool was created).  A verify job
    // has only t_submit, t_prove_start (its prelude's start) and t_done; everything else of it stays zero.
    starkhip_ticket_info_t info = {};
    Job() { info.leaf_hash_group = 1; }
};

int witness_limbs(int air);  // operands of `air`'s generator as u32 limbs (starkhip_pool_submit_witness); -1: it has none
// a witness job's recording on `tt` threads: its public inputs and its log (the toy AIR: plain rows); on failure nothing is kept
int record_witness(Job* j, int tt);
// Expected length of a small proof, for ordering only: the permutations per leaf of its commitment; trivial recordings first.
unsigned long small_rank(const Job* j);
// the queued recording a generator thread takes next; `big_wanted`: the pool's big contexts plus the recordings made ahead of them
std::deque<Job*>::iterator pick_recording(std::deque<Job*>& q_gen, size_t big_recordings_started, size_t big_wanted);
// the job of its class's queue that a context takes, q.end() when it should leave them all to others; `idle`: idle contexts of the
// class by the AIR they proved last
std::deque<Job*>::iterator pick_job(std::deque<Job*>& q, int last_air, const std::map<int, int>& idle, bool big);

struct Pool;
struct PoolLoad {
    double prove, verify;  // sums of air_cost / air_verify_cost over the jobs that are not done
    unsigned big_open;     // FinalExp-class jobs that are not done
};
PoolLoad pool_load(Pool* p);
void pool_set_pools_on_device(Pool* p, unsigned n);  // a multi-device handle was given this pool's ordinal n times

}  // namespace starkhip
