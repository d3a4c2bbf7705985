"""The reference's minimal perfect hash (pkg/mph/mph.go) restated in Python: hash, Load, Get, Store and Build, the last with a Go
1.14 sort.Slice of its own (src/sort/zfuncversion.go: quickSort_func and its helpers, driven by a less and a swap callback on
positions).  tests/gosort.py sorts keys by `<` and is left as it is; mph.Build's less is `len(b[i]) >= len(b[j])`, which is not
strict, so the order of equal buckets is whatever this particular sort leaves — and that order decides which free slots the
greedy gives to whom.  Up to 12 buckets the reference's own file tests/golden/lm/test.lm pins it; above that, two restatements
(this one and suggest_amd/csrc/lm_store.cpp) agreeing is all there is.  Test infrastructure."""
import struct

MASK = 0xFFFFFFFF
FREE = 0xFFFFFFFF


def mph_hash(seed, word):
    h = seed if seed else 2166136261
    for c in word:
        h = (h * 16777619) & MASK
        h ^= c
    return h


def load(data):
    """mph.Load over the bytes of a section -> (values, auxiliary, bytes read)"""
    n, = struct.unpack_from("<I", data, 0)
    values = list(struct.unpack_from("<%dI" % n, data, 4))
    s, = struct.unpack_from("<I", data, 4 + 4 * n)
    auxiliary = list(struct.unpack_from("<%di" % s, data, 8 + 4 * n))
    return values, auxiliary, 8 + 4 * (n + s)


def store(values, auxiliary):
    return struct.pack("<I%dI" % len(values), len(values), *values) + struct.pack("<I%di" % len(auxiliary), len(auxiliary), *auxiliary)


def get(values, auxiliary, word):
    d = auxiliary[mph_hash(0, word) % len(auxiliary)]
    if d < 0:
        return values[-d - 1]
    return values[mph_hash(d, word) % len(values)]


def go_sort_slice(n, less, swap):
    """sort.Slice of Go 1.14 over positions 0 .. n"""

    def insertion_sort(a, b):
        for i in range(a + 1, b):
            j = i
            while j > a and less(j, j - 1):
                swap(j, j - 1)
                j -= 1

    def sift_down(lo, hi, first):
        root = lo
        while True:
            child = 2 * root + 1
            if child >= hi:
                return
            if child + 1 < hi and less(first + child, first + child + 1):
                child += 1
            if not less(first + root, first + child):
                return
            swap(first + root, first + child)
            root = child

    def heap_sort(a, b):
        first, lo, hi = a, 0, b - a
        i = (hi - 1) // 2
        while i >= 0:
            sift_down(i, hi, first)
            i -= 1
        i = hi - 1
        while i >= 0:
            swap(first, first + i)
            sift_down(lo, i, first)
            i -= 1

    def median_of_three(m1, m0, m2):
        if less(m1, m0):
            swap(m1, m0)
        if less(m2, m1):
            swap(m2, m1)
            if less(m1, m0):
                swap(m1, m0)

    def do_pivot(lo, hi):
        m = (lo + hi) >> 1
        if hi - lo > 40:
            s = (hi - lo) // 8
            median_of_three(lo, lo + s, lo + 2 * s)
            median_of_three(m, m - s, m + s)
            median_of_three(hi - 1, hi - 1 - s, hi - 1 - 2 * s)
        median_of_three(lo, m, hi - 1)
        pivot = lo
        a, c = lo + 1, hi - 1
        while a < c and less(a, pivot):
            a += 1
        b = a
        while True:
            while b < c and not less(pivot, b):
                b += 1
            while b < c and less(pivot, c - 1):
                c -= 1
            if b >= c:
                break
            swap(b, c - 1)
            b += 1
            c -= 1
        protect = hi - c < 5
        if not protect and hi - c < (hi - lo) // 4:
            dups = 0
            if not less(pivot, hi - 1):
                swap(c, hi - 1)
                c += 1
                dups += 1
            if not less(b - 1, pivot):
                b -= 1
                dups += 1
            if not less(m, pivot):
                swap(m, b - 1)
                b -= 1
                dups += 1
            protect = dups > 1
        if protect:
            while True:
                while a < b and not less(b - 1, pivot):
                    b -= 1
                while a < b and less(a, pivot):
                    a += 1
                if a >= b:
                    break
                swap(a, b - 1)
                a += 1
                b -= 1
        swap(pivot, b - 1)
        return b - 1, c

    def quick_sort(a, b, max_depth):
        while b - a > 12:
            if max_depth == 0:
                heap_sort(a, b)
                return
            max_depth -= 1
            mlo, mhi = do_pivot(a, b)
            if mlo - a < b - mhi:
                quick_sort(a, mlo, max_depth)
                a = mhi
            else:
                quick_sort(mhi, b, max_depth)
                b = mlo
        if b - a > 1:
            for i in range(a + 6, b):
                if less(i, i - 6):
                    swap(i, i - 6)
            insertion_sort(a, b)

    depth, i = 0, n
    while i > 0:
        depth += 1
        i >>= 1
    quick_sort(0, n, depth * 2)


def build(words):
    """mph.Build over the words (bytes) in id order -> (values, auxiliary)"""
    size = len(words)
    buckets = [[] for _ in range(size)]
    values = []
    for key, w in enumerate(words):
        buckets[mph_hash(0, w) % size].append(key)
        values.append(FREE)
    auxiliary = [0] * size

    def less(i, j):
        return len(buckets[i]) >= len(buckets[j])

    def swap(i, j):
        buckets[i], buckets[j] = buckets[j], buckets[i]

    go_sort_slice(size, less, swap)
    bucket_iter = 0
    for bucket in buckets:
        if len(bucket) <= 1:
            break
        d, item, slots = 1, 0, []
        while item < len(bucket):
            slot = mph_hash(d, words[bucket[item]]) % size
            if values[slot] != FREE or slot in slots:
                d += 1
                item = 0
                slots = []
            else:
                slots.append(slot)
                item += 1
        auxiliary[mph_hash(0, words[bucket[0]]) % size] = d
        for i, key in enumerate(bucket):
            values[slots[i]] = key
        bucket_iter += 1
    free_slots = [i for i, v in enumerate(values) if v == FREE]
    for bucket in buckets[bucket_iter:]:
        if not bucket or not free_slots:
            break
        slot = free_slots.pop()
        auxiliary[mph_hash(0, words[bucket[0]]) % size] = -slot - 1
        values[slot] = bucket[0]
    return values, auxiliary
