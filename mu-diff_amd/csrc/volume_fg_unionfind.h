// find and union of the connected-component labelling of --foreground (volume_foreground.hip).  This header
// also compiles as plain host C++ (scripts/fg_unionfind_check.cpp drives it on the CPU under the address and undefined-behaviour
// sanitizers): the memory policy M says how a word is loaded and how a minimum is merged into it.
//
// parent[] holds, for a member voxel i, an index of the same component, and -1 for every other voxel.
// THE INVARIANT: parent[i] <= i at all times (a root has parent[i] == i).  It holds after the initialisation (parent[i] = i) and
// every write is a minimum of the stored value and a smaller index, so it can never break.  Every step of fg_find moves to a
// strictly smaller index and every retry of fg_union continues from a strictly smaller index: both end after at most i steps, whatever
// other threads do meanwhile and whatever stale value a load returns (a stale value is an earlier parent: it belongs to the same
// component and obeys the invariant too).  No loop waits for another thread's progress.  The loops test `<`, not `!=`, so they also
// end on memory that does not hold a forest at all.  The root of a finished tree is the smallest index of its component.
#pragma once

#if defined(__HIPCC__)
#define FG_HD __host__ __device__ __forceinline__
#else
#define FG_HD inline
#endif

// M::load(const int* p) -> the word; M::fetch_min(int* p, int v) -> the word before *p = min(*p, v), atomically
template <class M>
FG_HD int fg_find(const int* parent, int i) {
  int p = M::load(parent + i);
  while ((unsigned)p < (unsigned)i) {            // p < i: descend (a -1 never enters: it is the largest unsigned)
    i = p;
    p = M::load(parent + i);
  }
  return i;
}

// joins the components of the member voxels a and b
template <class M>
FG_HD void fg_union(int* parent, int a, int b) {
  for (;;) {
    a = fg_find<M>(parent, a);
    b = fg_find<M>(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = M::fetch_min(parent + b, a);   // a < b: parent[b] <= b stays true
    if ((unsigned)old >= (unsigned)b) return;      // b was a root and now hangs below a
    b = old;                                       // b had been linked below old < b meanwhile: a and old are still to be joined
  }
}

struct fg_host_memory {                            // one thread, plain words
  static inline int load(const int* p) { return *p; }
  static inline int fetch_min(int* p, int v) {
    const int old = *p;
    if (v < old) *p = v;
    return old;
  }
};
