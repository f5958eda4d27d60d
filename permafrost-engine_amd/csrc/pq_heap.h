// pq_heap.h -- the binary heap of lib/public/pqueue.h (:109-208) replayed operation for operation by ONE lane: arbitrary
// float priorities, a push may lie below the last pop.  What decides the order of equal priorities there decides it here:
// the push sifts up while the parent is strictly GREATER (:186), the pop moves the last node to the root and sinks a
// HOLE (_balance, :109-130): the node to place stays at nodes[size + 1], a child replaces it only when strictly LESS, the
// right child is compared against the winner so far.  (The LOS kernel's heap is a two-priority specialisation of the same
// rules, los_kernels.hip; this is the general one.)  Nodes are 1-based as in the reference: prio / data hold cap + 2
// elements, [0] unused, [size + 1] read by the pop.  Free of device variables, so any unit may include it.
#pragma once
#include <stdint.h>

struct pq_heap { float *prio; uint32_t *data; int size, cap; };

// pq_push (:165): false when the heap is full (the reference grows its array; the caller's answer is "not decided")
__device__ __forceinline__ bool pq_heap_push(pq_heap &h, float in_prio, uint32_t in)
{
    if(h.size + 1 > h.cap) return false;
    int curr = h.size + 1, parent = curr / 2;
    while(curr > 1 && h.prio[parent] > in_prio) {
        h.prio[curr] = h.prio[parent]; h.data[curr] = h.data[parent];
        curr = parent;
        parent = parent / 2;
    }
    h.prio[curr] = in_prio; h.data[curr] = in;
    h.size++;
    return true;
}

// pq_pop (:198) with _balance(1): the caller has checked size > 0
__device__ __forceinline__ uint32_t pq_heap_pop(pq_heap &h)
{
    const uint32_t out = h.data[1];
    h.prio[1] = h.prio[h.size]; h.data[1] = h.data[h.size];
    h.size--;
    int root = 1;
    while(root != h.size + 1) {
        int target = h.size + 1;
        const int left = root * 2, right = left + 1;
        if(left <= h.size && h.prio[left] < h.prio[target]) target = left;
        if(right <= h.size && h.prio[right] < h.prio[target]) target = right;
        h.prio[root] = h.prio[target]; h.data[root] = h.data[target];
        root = target;
    }
    return out;
}
