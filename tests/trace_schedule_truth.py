"""The traversal kernel's hand-out of rays to waves, restated in plain Python integers: no library import, nothing of the kernel's but its text.

fermat_amd/csrc/fpt_trace_kernel.inc gives the rays [0, n) of a launch to the waves of a persistent grid (`blocks` blocks of 256 threads = 4 waves each):

  waves       = 4 blocks
  static      iff n <= 64 waves: wave w owns the fixed batch [64 w, min(64 w + 64, n)) -- nothing when 64 w >= n -- and no counter is touched
  shard_size  = ceil(n / 8); shard k = [sb, se) with sb = k shard_size and se = (k + 1) shard_size, the LAST shard ending at n
  chunk       = clamp(((n // (2 waves)) + 63) & ~63, 64, 256)
  a draw      on shard k: old = atomicAdd(counter[k], chunk); base = sb + old; accepted iff base < se, and then it hands out [base, min(base + chunk, se))
  a wave      starts on shard (wave id % 8), draws whenever its chunk is used up, moves to the next shard (cyclically) after a refused draw, and is dry -- it
              draws no more -- after a round of eight refused draws, one on every shard

The old values of the draws on one shard are 0, chunk, 2 chunk, ... whoever draws and in whatever order, so the accepted ranges are a function of (n, blocks)
alone: covers_once() lists them and checks that they tile [0, n).  final_counters() bounds what the eight counters hold after a finished launch, which is what
tests/test_trace_schedule.py reads back from the device to know that a capped launch really ran on tickets and really exhausted every shard.
"""

SHARDS = 8
WAVE = 64
WAVES_PER_BLOCK = 4          # TRACE_BLOCK = 256 threads
CHUNK_MAX = 256              # FPT_CHUNK_MAX
REFILL_MIN = 16              # FPT_REFILL_MIN: a wave refills once this many lanes are idle


def waves_of(blocks):
    return WAVES_PER_BLOCK * blocks


def launch_blocks(n, cap):
    """the grid of an fpt_rt_trace* launch of n rays on a context whose persistent grid is `cap` blocks: min(cap, ceil(n / 256)) (rt_launch, fpt_api.cpp)"""
    return min(cap, (n + 255) // 256)


def is_static(n, blocks):
    return n <= WAVE * waves_of(blocks)


def chunk_of(n, blocks):
    c = ((n // (2 * waves_of(blocks))) + 63) & ~63
    return max(64, min(CHUNK_MAX, c))


def shard_size_of(n):
    return (n + SHARDS - 1) // SHARDS


def shards(n):
    """[(sb, se)] of the eight shards, as the kernel computes them (for small n a shard may begin past n: see last_shard_begins_inside)"""
    ss = shard_size_of(n)
    return [(k * ss, n if k + 1 == SHARDS else (k + 1) * ss) for k in range(SHARDS)]


def last_shard_begins_inside(n):
    """7 ceil(n / 8) <= n: the first seven shards end at or before n.  Where it fails, shard 6 (or an earlier one) ends past n and its draws would hand out rays
    that do not exist.  It holds for every n >= 49 (7 (n + 7) / 8 <= n iff n >= 49) and fails, for example, at n = 41 (7 * 6 = 42)."""
    return (SHARDS - 1) * shard_size_of(n) <= n


def accepted_ranges(n, blocks):
    """every range a launch hands out, as (begin, end, shard or None), in no particular order"""
    if is_static(n, blocks):
        return [(WAVE * w, min(WAVE * w + WAVE, n), None) for w in range(waves_of(blocks)) if WAVE * w < n]
    chunk = chunk_of(n, blocks)
    out = []
    for k, (sb, se) in enumerate(shards(n)):
        old = 0
        while sb + old < se:          # the draws that follow are refused: they only add to the counter
            out.append((sb + old, min(sb + old + chunk, se), k))
            old += chunk
    return out


def covers_once(n, blocks):
    """Under any order of draws the accepted ranges tile [0, n) exactly once and none ends past n.  Raises AssertionError otherwise; returns the number of ranges.

    A launch on tickets also needs last_shard_begins_inside(n); it is asserted here for the launch at hand, and check_small_n_stays_static() asserts that every n
    that can leave the static path at all has it -- so a later change of the static threshold cannot silently open the small-n case."""
    assert n >= 0 and blocks >= 1
    if not is_static(n, blocks):
        assert last_shard_begins_inside(n), "n = %d runs on tickets but 7 ceil(n / 8) > n: a shard ends past n" % n
    ranges = sorted(accepted_ranges(n, blocks))
    at = 0
    for b, e, k in ranges:
        assert b < e, "an empty range (%d, %d) is handed out, shard %s" % (b, e, k)
        assert e <= n, "the range (%d, %d) of shard %s ends past n = %d" % (b, e, k, n)
        assert b == at, "rays [%d, %d) are handed out %s (n = %d, %d blocks)" % (min(at, b), max(at, b), "twice" if b < at else "never", n, blocks)
        at = e
    assert at == n, "rays [%d, %d) are never handed out (%d blocks)" % (at, n, blocks)
    return len(ranges)


def check_small_n_stays_static():
    """The two facts behind covers_once's second property.  (1) The smallest launch that can leave the static path -- one block, n = 64 * 4 + 1 = 257 -- is far
    above 49, from where 7 ceil(n / 8) <= n always holds.  (2) Below, it does fail: every such n is < 49 < 56, and all of them are static on every grid."""
    smallest_on_tickets = WAVE * waves_of(1) + 1
    assert smallest_on_tickets == 257 and not is_static(smallest_on_tickets, 1) and is_static(smallest_on_tickets - 1, 1)
    failing = [n for n in range(1, 4096) if not last_shard_begins_inside(n)]
    assert failing and max(failing) == 41 and max(failing) < 56 <= smallest_on_tickets, failing
    assert all(last_shard_begins_inside(n) for n in range(49, 1 << 16))
    assert all(is_static(n, blocks) for n in failing for blocks in (1, 2, 3, 1792))
    return failing


def final_counters(n, blocks):
    """What must hold of the eight counters after a finished launch of n rays on `blocks` blocks: dict(static, chunk, lo[8], hi[8]).

    Static: the kernel touches no counter, and the host zeroed them before the launch: lo = hi = 0.
    On tickets, counter k = chunk x (the number of draws on shard k), so it is a multiple of chunk, and
      * accepted draws: exactly ceil(len_k / chunk), len_k = se - sb: the accepted old values are 0, chunk, ... below len_k;
      * refused draws: at least `waves`.  A wave leaves the kernel only when it is dry: the refill runs whenever all 64 lanes are idle and the wave is not dry,
        and it either hands lane 0 a ray or ends dry.  It ends dry only by a round of eight refused draws, one on every shard.  So every wave of the grid adds
        one refused draw to every shard;
      * refused draws: at most 2 `waves`.  A shard that refuses is exhausted and stays so.  A wave that is refused on shard k in a round that another shard j
        then ends with an accepted draw stays on j; it meets k again only after refusals on j, j + 1, ..., k - 1, and the shards after k up to j were refused
        in the earlier round: that second round refuses eight times and is the wave's last.
    Hence lo_k = chunk (ceil(len_k / chunk) + waves) <= counter k <= hi_k = chunk (ceil(len_k / chunk) + 2 waves).  lo_k > len_k: every shard is exhausted."""
    if is_static(n, blocks):
        return dict(static=True, chunk=0, lo=[0] * SHARDS, hi=[0] * SHARDS)
    chunk, waves = chunk_of(n, blocks), waves_of(blocks)
    need = [(se - sb + chunk - 1) // chunk for sb, se in shards(n)]
    return dict(static=False, chunk=chunk, lo=[chunk * (a + waves) for a in need], hi=[chunk * (a + 2 * waves) for a in need])


def check_counters(n, blocks, counters):
    """counters (eight integers read back after a launch) against final_counters(n, blocks); raises AssertionError naming the shard"""
    want = final_counters(n, blocks)
    got = [int(c) for c in counters]
    assert len(got) == SHARDS
    for k in range(SHARDS):
        where = "shard %d of n = %d on %d blocks: counter %d" % (k, n, blocks, got[k])
        if want["static"]:
            assert got[k] == 0, where + " on the static path"
            continue
        assert got[k] % want["chunk"] == 0, where + " is no multiple of the chunk %d" % want["chunk"]
        assert got[k] >= want["lo"][k], where + " < %d: the shard was not exhausted by every wave" % want["lo"][k]
        assert got[k] <= want["hi"][k], where + " > %d: more refused draws than two per wave" % want["hi"][k]
    return want


def simulate(n, blocks, order):
    """One finished launch on tickets with the waves' draws interleaved by `order` (an iterable of wave ids, consumed until every wave is dry; a dry wave's turn is
    skipped): each turn is one refill's draw -- a round of up to eight atomics.  Returns (ranges handed out as (begin, end, wave), the eight counters)."""
    assert not is_static(n, blocks)
    chunk, waves, sh = chunk_of(n, blocks), waves_of(blocks), shards(n)
    counter = [0] * SHARDS
    shard = [w % SHARDS for w in range(waves)]
    dry = [False] * waves
    out = []
    for w in order:
        if all(dry):
            break
        if dry[w]:
            continue
        got = None
        for _ in range(SHARDS):
            sb, se = sh[shard[w]]
            base = sb + counter[shard[w]]
            counter[shard[w]] += chunk
            if base < se:
                got = (base, min(base + chunk, se), w)
                break
            shard[w] = (shard[w] + 1) % SHARDS
        if got is None:
            dry[w] = True
        else:
            out.append(got)
    assert all(dry), "the order ended before every wave was dry"
    return out, counter


def refill(idle_lanes, c_next, c_end):
    """The partial-wave refill: the idle lanes (a sorted list of lane numbers) take the rays c_next + rank, rank = the lane's position among the idle lanes, while
    rank < c_end - c_next.  Returns ({lane: ray}, the new c_next)."""
    avail = c_end - c_next
    given = {lane: c_next + rank for rank, lane in enumerate(idle_lanes) if rank < avail}
    return given, c_next + min(len(idle_lanes), avail)


SELF_CHECK_CASES = [(256, 1), (257, 1), (768, 3), (769, 3), (2049, 1), (2049, 3), (5000, 1), (5000, 3), (458752, 1792), (458753, 1792)]


def self_check():
    """hand-made cases; returns what it found for the caller to look at"""
    check_small_n_stays_static()
    report = {}
    for n, blocks in SELF_CHECK_CASES:
        report[n, blocks] = (covers_once(n, blocks), is_static(n, blocks), chunk_of(n, blocks))
    # the static threshold sits exactly between each pair
    assert is_static(256, 1) and not is_static(257, 1) and is_static(768, 3) and not is_static(769, 3) and is_static(458752, 1792) and not is_static(458753, 1792)
    # chunks worked out by hand: 257 // 8 = 32 -> 64; 769 // 24 = 32 -> 64; 2049 // 24 = 85 -> 128; 2049 // 8 = 256 -> 256; 5000 // 8 = 625 -> 640 -> 256; 458753 // 14336 = 32 -> 64
    assert [chunk_of(*c) for c in ((257, 1), (769, 3), (2049, 3), (2049, 1), (5000, 1), (5000, 3), (458753, 1792))] == [64, 64, 128, 256, 256, 256, 64]
    # 257 rays, one block: shards of 33 rays, the last [231, 257) of 26; one accepted draw each; 4 waves -> each counter in [64 (1 + 4), 64 (1 + 8)]
    assert shards(257) == [(0, 33), (33, 66), (66, 99), (99, 132), (132, 165), (165, 198), (198, 231), (231, 257)]
    f = final_counters(257, 1)
    assert not f["static"] and f["chunk"] == 64 and f["lo"] == [320] * 8 and f["hi"] == [576] * 8
    # 5000 rays, three blocks: shards of 625 = 3 draws of 256; 12 waves -> [256 * 15, 256 * 27]
    f = final_counters(5000, 3)
    assert f["chunk"] == 256 and f["lo"] == [3840] * 8 and f["hi"] == [6912] * 8
    assert final_counters(768, 3) == dict(static=True, chunk=0, lo=[0] * 8, hi=[0] * 8)
    # the grid of an fpt_rt_trace* launch: at cap 3, 257 and 320 rays run on two blocks and 768 on three -- static; 769 is the first on tickets
    assert [launch_blocks(n, 3) for n in (256, 257, 320, 768, 769, 5000)] == [1, 2, 2, 3, 3, 3] and [launch_blocks(n, 1) for n in (256, 257)] == [1, 1]
    assert [is_static(n, launch_blocks(n, 3)) for n in (256, 257, 320, 768, 769, 2049, 5000)] == [True, True, True, True, False, False, False]
    assert [is_static(n, launch_blocks(n, 1)) for n in (256, 257, 320, 768, 769, 2049, 5000)] == [True, False, False, False, False, False, False]
    # any order of draws: the same tiling, counters inside the bounds.  Round-robin, one wave racing ahead, and the waves in reverse
    for n, blocks in ((257, 1), (769, 3), (2049, 3), (5000, 1), (5000, 3)):
        waves = waves_of(blocks)
        orders = {"round robin": [w for _ in range(4 * n) for w in range(waves)],
                  "wave 0 first": [0] * (4 * n) + [w for _ in range(4 * n) for w in range(waves)],
                  "reversed": [w for _ in range(4 * n) for w in reversed(range(waves))]}
        for name, order in orders.items():
            got, counter = simulate(n, blocks, order)
            assert sorted((b, e) for b, e, _ in got) == sorted((b, e) for b, e, _ in accepted_ranges(n, blocks)), (n, blocks, name)
            check_counters(n, blocks, counter)
        # with 4 waves (one block) no wave starts on shards 4..7: they are reached by stealing only
        if blocks == 1:
            got, _ = simulate(n, blocks, orders["round robin"])
            assert all(any(b >= sb and e <= se for b, e, _ in got) for sb, se in shards(n)[4:])
    # check_counters has teeth: a shard one wave short of exhausted, a counter off the chunk grid, a counter on the static path
    f = final_counters(5000, 1)
    for bad in ([c - 256 if k == 5 else c for k, c in enumerate(f["lo"])], [c + 64 if k == 0 else c for k, c in enumerate(f["lo"])]):
        try:
            check_counters(5000, 1, bad)
        except AssertionError:
            continue
        raise AssertionError("check_counters accepted %s" % bad)
    try:
        check_counters(256, 1, [0, 0, 64, 0, 0, 0, 0, 0])
    except AssertionError:
        pass
    else:
        raise AssertionError("check_counters accepted a counter on the static path")
    # the refill by rank: 20 idle lanes, 5 rays left -> the 5 lowest idle lanes; 70 rays left -> all 20
    idle = list(range(3, 63, 3))
    assert refill(idle, 100, 105) == ({3: 100, 6: 101, 9: 102, 12: 103, 15: 104}, 105)
    given, nxt = refill(idle, 100, 170)
    assert nxt == 120 and sorted(given.values()) == list(range(100, 120)) and sorted(given) == idle
    return report
