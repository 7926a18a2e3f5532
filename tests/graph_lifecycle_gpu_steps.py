"""GPU steps of tests/test_graph_lifecycle_gpu.py, each run in a child process of its own under a time limit:
    python tests/graph_lifecycle_gpu_steps.py open_close | failed_create | regrow | resize
The graph handle (dbgk_handle) owns its device memory, pinned memory, events and streams through the owners of
csrc/dbgk_host_stage.h: these steps open and close every shape of it, let creates fail after the handle exists, grow the buffers that
grow with a batch, and resize the table.  Every table is compared with the oracle's or with a second handle that never took the path.
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PART_SLOTS = 70000000      # the PARTITION engine needs 2^26 slots and more
TRACK_MESSAGE = "DBGK_FLAG_TRACK_FIRST_SEEN needs the DIRECT engine"


def make_reads(rng, n, lo, hi, genome):
    """n reads of lo..hi bases cut from `genome` (a uint8 array of ACGT), so that k-mers repeat between reads"""
    lens = rng.integers(lo, hi + 1, n)
    starts = rng.integers(0, len(genome) - hi, n)
    return [genome[s:s + ln].tobytes() for s, ln in zip(starts, lens)]


def genome_of(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]


def oracle_nodes(capi, O, batches, k=31):
    ref = O.build_graph(files_mem=list(batches), k=k, init_hash_size=0.001, threads=1)
    return ref, ref.nodes.astype(capi.NODE_DTYPE)


def check_graph(capi, g, ref, want, what):
    st = g.finalize()
    assert (int(st.total_reads), int(st.total_kmers), int(st.count)) == (ref.total_reads, ref.total_kmers, ref.count), \
        (what, int(st.total_reads), int(st.total_kmers), int(st.count), ref.total_reads, ref.total_kmers, ref.count)
    assert np.array_equal(g.export_sorted(), want), (what, "nodes differ from the oracle's")
    return int(st.count)


def shapes(capi):
    """every shape of the handle -> a call that makes one on device 0"""
    prime = capi.find_next_prime_ref
    G = capi.Graph
    return {
        "direct": lambda: G(k=31, table_slots=prime(1000000), engine=capi.ENGINE_DIRECT),
        "direct_first_seen": lambda: G(k=31, table_slots=prime(1000000), engine=capi.ENGINE_DIRECT, flags=capi.FLAG_TRACK_FIRST_SEEN),
        "partition": lambda: G(k=31, table_slots=prime(PART_SLOTS), engine=capi.ENGINE_PARTITION, expected_kmers=100000),
        "partition_one_shard": lambda: G(k=31, table_slots=prime(PART_SLOTS), engine=capi.ENGINE_PARTITION, expected_kmers=100000, shard_count=1),
        "kfreq_direct": lambda: G(k=9, table_slots=0, engine=capi.ENGINE_KFREQ),
        "kfreq_hashed": lambda: G(k=11, table_slots=0, engine=capi.ENGINE_KFREQ, expected_kmers=100000),
        "kfreq_blocks": lambda: G(k=13, table_slots=0, engine=capi.ENGINE_KFREQ, expected_kmers=100000),
        "seedidx": lambda: G(k=31, table_slots=prime(1000000), engine=capi.ENGINE_SEEDIDX),
        "wide_atomic": lambda: G(k=63, table_slots=prime(100000), engine=capi.ENGINE_WIDE),
        "wide_records": lambda: G(k=63, table_slots=prime(1 << 26), engine=capi.ENGINE_WIDE, expected_kmers=100000),
    }


def open_close():
    """one handle of every shape made and closed twice; all of them open at once and closed in the order they were made;
    dbgk_destroy refuses a null handle"""
    from dbg_assembly_amd import capi
    res = {}
    for name, make in shapes(capi).items():
        for _ in range(2):
            g = make()
            assert g._h
            if name == "wide_records":
                assert g.store_room()[1] > 0, "the WIDE handle does not collect records"
            if name.startswith("partition"):
                assert g.store_room()[1] == 100000
            g.close()
            assert not g._h
        res[name] = "closed"
    together = [make() for make in shapes(capi).values()]
    for g in together:
        g.close()
    res["together"] = len(together)
    res["destroy_null"] = capi.lib().dbgk_destroy(None)
    return res


def failed_create():
    """creates that fail after the handle exists, or just before: *out is null, and a good create on device 0 works afterwards and
    gives the oracle's table"""
    from dbg_assembly_amd import capi
    from oracle import oracle_py as O
    L = capi.lib()
    n_dev = L.dbgk_device_count()
    assert n_dev >= 1
    rng = np.random.default_rng(5)
    batch = O.pack_reads(make_reads(rng, 2000, 31, 90, genome_of(rng, 20000)))
    ref, want = oracle_nodes(capi, O, [batch])
    prime = capi.find_next_prime_ref
    # Config(k, max_read_len, table_slots, device, engine, max_batch_bases, expected_kmers, shard_count, shard_index, flags, n_passes)
    bad = {
        "first_seen_on_partition": capi.Config(31, 250, prime(PART_SLOTS), 0, capi.ENGINE_PARTITION, 0, 100000, 0, 0, capi.FLAG_TRACK_FIRST_SEEN, 0),
        "device_past_the_last": capi.Config(31, 250, prime(1000000), n_dev, capi.ENGINE_DIRECT, 0, 0, 0, 0, 0, 0),
        "device_minus_1": capi.Config(31, 250, prime(1000000), -1, capi.ENGINE_DIRECT, 0, 0, 0, 0, 0, 0),
        "sharded_small_table": capi.Config(31, 250, prime(1000000), 0, capi.ENGINE_PARTITION, 0, 100000, 2, 0, 0, 0),
    }
    res = {}
    for name, cfg in bad.items():
        h = ctypes.c_void_p(1)
        res[name] = {"status": L.dbgk_create(ctypes.byref(cfg), ctypes.byref(h))}
        if name == "first_seen_on_partition":
            res[name]["error"] = L.dbgk_last_error().decode()
        assert not h.value, name
        with capi.Graph(k=31, table_slots=prime(1000000), engine=capi.ENGINE_DIRECT, device=0) as g:
            g.push_reads(*batch)
            res[name]["nodes_after"] = check_graph(capi, g, ref, want, name)
    return res


def regrow():
    """one PARTITION handle with staging batches of 2^17 bases (cap_reads = 9216): device batches of mixed read lengths small, large
    enough to grow the start / dead bitmaps and the packed image, small, larger again and of more reads than cap_reads (the prefix
    scratch grows); then small / large / small through push_reads_packed_device and through push_reads_packed_uniform_device (reads of
    20 windows, which need offsets made on the device: more than cap_reads of them in the large batch)"""
    from dbg_assembly_amd import capi
    from oracle import oracle_py as O
    rng = np.random.default_rng(17)
    genome = genome_of(rng, 60000)
    mixed = [make_reads(rng, n, lo, hi, genome) for n, lo, hi in ((60, 35, 80), (3000, 40, 120), (50, 31, 70), (10000, 31, 70))]
    packed = [make_reads(rng, n, lo, hi, genome) for n, lo, hi in ((40, 35, 90), (3500, 40, 110), (30, 33, 60))]
    uniform = [make_reads(rng, n, ln, ln, genome) for n, ln in ((48, 50), (9500, 48), (32, 50))]
    batches = [O.pack_reads(r) for r in mixed + packed + uniform]
    assert len(mixed[3]) > 9216 and int(batches[0][1][-1]) < 6000 and int(batches[1][1][-1]) > 200000 and int(batches[3][1][-1]) > int(batches[1][1][-1])
    ref, want = oracle_nodes(capi, O, batches)
    res = {}
    with capi.Graph(k=31, table_slots=capi.find_next_prime_ref(PART_SLOTS), engine=capi.ENGINE_PARTITION,
                    expected_kmers=sum(int(b[1][-1]) for b in batches), max_batch_bases=1 << 17) as g:
        held = []

        def on_device(arr):
            buf = capi.DeviceBuffer(g, arr.nbytes + 64)
            buf.from_host(arr)
            held.append(buf)
            return buf.ptr

        for i, (bases, offsets) in enumerate(batches[:4]):
            if i == 3:
                g.reset_timings()   # (the log of level-1 forms starts again: what follows is this batch's)
            g.push_reads_device(on_device(bases), on_device(offsets), len(offsets) - 1, int(offsets[-1]))
        g.sync()
        forms = g.l1_forms()
        res["forms_of_the_large_batch"] = forms
        assert any(f.startswith("family=prefix ") for f in forms), forms
        assert g.timings().prefix_launches >= 1
        for bases, offsets in batches[4:7]:
            words, _ = capi.pack_bases(bases)
            g.push_reads_packed_device(on_device(words), on_device(offsets), len(offsets) - 1, int(offsets[-1]))
        for bases, offsets in batches[7:]:
            words, _ = capi.pack_bases(bases)
            g.push_reads_packed_uniform_device(on_device(words), len(offsets) - 1, int(offsets[1]))
        res["nodes"] = check_graph(capi, g, ref, want, "regrow")
        for buf in held:
            buf.free()
    return res


def resize():
    """DIRECT with first-seen tracking: push, a resize that is refused (table full), a resize to twice the size, push, finalize -- the
    nodes and their first-seen order are those of a handle made at the final size.  PARTITION: a size the engine cannot take is refused
    and the handle goes on; a resize before anything was pushed and one after a flush give the oracle's table."""
    from dbg_assembly_amd import capi
    from oracle import oracle_py as O
    rng = np.random.default_rng(23)
    genome = genome_of(rng, 50000)
    halves = [O.pack_reads(make_reads(rng, 1500, 31, 120, genome)) for _ in range(2)]
    ref, want = oracle_nodes(capi, O, halves)
    prime = capi.find_next_prime_ref
    res = {}
    small, large = prime(1000000), prime(2 * prime(1000000))

    def tracked(size):
        return capi.Graph(k=31, table_slots=size, engine=capi.ENGINE_DIRECT, flags=capi.FLAG_TRACK_FIRST_SEEN)

    with tracked(small) as g, tracked(large) as never_resized:
        g.push_reads(*halves[0])
        try:
            g.resize_table(1009)
            res["direct_too_small"] = capi.OK
        except capi.DbgkError as e:
            res["direct_too_small"] = e.status
        g.resize_table(large)
        g.push_reads(*halves[1])
        for b in halves:
            never_resized.push_reads(*b)
        res["direct_nodes"] = check_graph(capi, g, ref, want, "direct, resized")
        check_graph(capi, never_resized, ref, want, "direct, made at the final size")
        (nodes_a, pos_a), (nodes_b, pos_b) = g.export_first_seen_order(), never_resized.export_first_seen_order()
        assert len(nodes_a) == ref.count - 1 and np.array_equal(nodes_a, nodes_b) and np.array_equal(pos_a, pos_b), "first-seen order"

    with capi.Graph(k=31, table_slots=prime(PART_SLOTS), engine=capi.ENGINE_PARTITION, expected_kmers=1 << 20) as g:
        try:
            g.resize_table(1000003)
            res["partition_unfit"] = capi.OK
        except capi.DbgkError as e:
            res["partition_unfit"] = e.status
        for b in halves:
            g.push_reads(*b)
        res["partition_nodes_after_refusal"] = check_graph(capi, g, ref, want, "partition, after a refused resize")

    with capi.Graph(k=31, table_slots=prime(PART_SLOTS), engine=capi.ENGINE_PARTITION, expected_kmers=1 << 20) as g:
        g.resize_table(prime(PART_SLOTS + 30000000))     # nothing pushed yet
        g.push_reads(*halves[0])
        g.flush()
        assert g.store_room()[0] == 0
        g.resize_table(prime(2 * PART_SLOTS))            # the table holds the nodes of the first half
        g.push_reads(*halves[1])
        res["partition_nodes"] = check_graph(capi, g, ref, want, "partition, resized twice")
    return res


if __name__ == "__main__":
    print(json.dumps({"open_close": open_close, "failed_create": failed_create, "regrow": regrow, "resize": resize}[sys.argv[1]]()))
