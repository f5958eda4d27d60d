// tests/hostsim/pq_heap_sim.cpp -- TEST INFRASTRUCTURE ONLY: csrc/pq_heap.h compiled for the host (one lane is all it
// needs) and driven by a script of pushes and pops, for tests/test_arrival_build_cpu.py.
#include <stdint.h>
#define __device__
#define __forceinline__ inline
#include "pq_heap.h"

// ops[i] >= 0: push (prio[i], ops[i]); ops[i] < 0: pop.  out[i]: 1 / 0 for a push that fitted / was refused, the popped
// datum for a pop (-1 from an empty heap, which the kernel never asks).  Returns the heap's size at the end.
extern "C" int pq_heap_script(int cap, int n, const int32_t *ops, const float *prio, int32_t *out, float *node_prio, uint32_t *node_data)
{
    pq_heap H;
    H.prio = node_prio; H.data = node_data; H.size = 0; H.cap = cap;
    for(int i = 0; i < n; i++) {
        if(ops[i] >= 0) out[i] = pq_heap_push(H, prio[i], (uint32_t)ops[i]) ? 1 : 0;
        else out[i] = H.size > 0 ? (int32_t)pq_heap_pop(H) : -1;
    }
    return H.size;
}
