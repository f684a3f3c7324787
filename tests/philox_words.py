"""The Philox key and counter words the sampling kernels are held to, and the ways a kernel could lose one of them.

TEST INFRASTRUCTURE, written for this repository's tests.  Every sampled number here is a Philox4x32-10 draw under the key (seed low, seed high) at the
counter (index inside the traversal, global traversal id b0 + i, iteration, stream tag).  A kernel that dropped or truncated one of those words would
still sample plausibly, so each GPU test that runs a wide word has a CPU guard (the test_*_ref.py of its restatement) asserting that its expectation
SEPARATES: the reference result at the wide word differs, in a quantity the GPU test compares exactly, from the result with that word narrowed in one
of the ways `narrowed` lists."""
M32 = 0xFFFFFFFF
WIDE_SEED = 0x9E3779B97F4A7C15     # both key words non-zero and different (tests/test_gpu_multi_mccfr.py's)
ITER_HI = 0xFFFFFFFF
ITER_B31 = 0x80000000              # bit 31 alone: a signed compare or an int32 argtype shows here, a 16-bit cast does too


def ids_of(b0, nb, wrap=1 << 32):
    """the global traversal ids b0 + i, computed modulo `wrap`"""
    return [(int(b0) + i) % wrap for i in range(nb)]


def word_cases(narrow_seed, nb, b0_last, small_iteration=5, small_b0=3):
    """(seed, iteration, b0) with one word wide at a time, then all of them at once; b0_last = the entry point's largest accepted b0 for nb"""
    return [(WIDE_SEED, small_iteration, small_b0), (narrow_seed, ITER_HI, small_b0), (narrow_seed, ITER_B31, small_b0),
            (narrow_seed, small_iteration, b0_last), (WIDE_SEED, ITER_HI, b0_last)]


def case_id(word):
    """pytest id of one word of a parametrised (seed, iteration, b0)"""
    return hex(word) if isinstance(word, int) else None


def narrowed(seed, iteration, b0, nb):
    """[(what, seed', iteration', ids')]: the words as a kernel that lost part of one would see them; only the variants that change a word"""
    ids = ids_of(b0, nb)
    out = [("the seed cut to its low 32 bits", seed & M32, iteration, ids)]
    for bits in (16, 31):
        m = (1 << bits) - 1
        out.append((f"the iteration cut to its low {bits} bits", seed, iteration & m, ids))
        out.append((f"b0 cut to its low {bits} bits", seed, iteration, ids_of(b0 & m, nb)))
    out.append(("b0 + i wrapped at 2^31", seed, iteration, ids_of(b0, nb, 1 << 31)))
    return [v for v in out if v[1:] != (seed, iteration, ids)]


# ---- Deep CFR traversals (tests/test_gpu_sdcfr.py, tests/test_gpu_chance_sdcfr.py; guarded by tests/test_sdcfr_policy_ref.py) -------------------------
def sd_last_b0(batch):
    """the single-deal entry points take any b0 and the solver passes rank * batch: the largest multiple of the batch whose last id b0 + batch - 1 is
    still below 2^32 (2^32 - batch where the batch divides 2^32)"""
    return ((1 << 32) // batch - 1) * batch


SD_SEED = 0x5C09A
SD_BATCH = 64                                  # the smallest batch of the vs-oracle family (test_traversal_on_other_deals_vs_oracle)
SD_WORD_CASES = word_cases(SD_SEED, SD_BATCH, sd_last_b0(SD_BATCH), small_iteration=3, small_b0=0)
SD_EXTREME = (WIDE_SEED, ITER_B31, None)       # b0 = sd_last_b0(batch) of the batch at hand: the tuple the form-against-form tests add to (SD_SEED, small, 0)
SD_FORM_BATCHES = (303, 1, 5, 67)              # the batches of those tests
# the chance form: six deals, batch 5; ids b0 + deal * batch + i.  The entry point accepts b0 <= 2^32 - 6 * batch
CH_SEED, CH_BATCH, CH_ITERATION = 0xD33C0F, 5, 3
CH_WIDE = (WIDE_SEED, ITER_B31, 1000, [3, 0, 5])                       # (seed, iteration, b0, deals)
CH_LAST = (CH_SEED, CH_ITERATION, (1 << 32) - 6 * CH_BATCH, [0, 1, 2, 3, 4, 5])
