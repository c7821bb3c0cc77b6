"""The bytes of the shared workloads, pinned.  The floors that the GPU tests assert (PAIR_FLOORS, RESCUE_FLOORS, STRAND_FLOORS, the
floors of the script, secondary and front tests) were confirmed once, with the naive chain on the CPU, for exactly these inputs; a
generator that drifts by one seed would leave those tests passing while they check something else.  Every digest is a SHA-256 over
the arrays a generator returns (for each its dtype, its shape and its bytes, in order), taken from the generators as they stood in
the test files before they were gathered in tests/chain_data.py and tests/front_data.py: the four copies of reads_of, the three
of the repeat text and the seven of text_of gave the same bytes wherever their arguments met."""
import hashlib

import numpy as np
import pytest

from tests import chain_data as cd
from tests import front_data as fd
from tests.helpers import pack


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + b":" + str(a.shape).encode() + b":")
        h.update(a.tobytes())
    return h.hexdigest()


def digest_of_meta(meta):
    return hashlib.sha256(repr([tuple(int(x) for x in t) for t in meta]).encode()).hexdigest()


TEXTS = {
    (4, 50_000): "44422d319a77366b050d99c5e60b4dfcff75bc8fbd439d011b988501227abd31",
    (20, 50_000): "e03f14c31b02464442a770b0b16058b4826f0ce710bceee9f4cb4fb3b9180d4e",
    (4, 100_000): "69c393ee6cf5c419b64b19580794111c1e51900f3af4636d11fbadcda27e2996",
}
# (workload, n_reads, meta, reverse_odd) -> (the reads, the side table): the arguments of the vote, align, script and strand-fold tests
READS = {
    ("dna4_k10", None, "plain", False): ("4e0b221d0eef060cbee1b103bbafc8de73c5fd6a5a6d3842dad8b11b42df1cdd", "4931af45d1d31b8d5df9701d95eca3672cea60460166459c850f4bdba7cac4ee"),
    ("aa20_k5", None, "plain", False): ("d72d45e5d1763b2332db58c6dcfc437490856a0e982f0b52c4b21e8fc60baf52", "46ca346b7421b75a2d6b4d1bf7fb338fba12e8f0b6d3104e1d09c893625e9eb9"),
    ("dna4_k5", None, "plain", False): ("5c6d26a41aba2ea4c58eb224dfb5a3df3db87c5c0f3033970c1b0981ec237c3d", "79279670cd9327ec3e0b61693373819a54c1d8392bbc681b6cd69b5001bd1a27"),
    ("dna4_k10", cd.N_READS, "bad", False): ("6c87e35acb295d4873bac10b144b2cb06f61aefb79615109ea18216680fcf9af", "769151069fc3f4db9f403ea5aedec30cd67d20a3399cf5c6da2f9fd3e7d9a3e6"),
    ("aa20_k5", cd.N_READS, "bad", False): ("c70f67f6e4dd933a7ebaaa372f9af0e63d7167ffdc6acee03970c3983abcc4b6", "a20b18f9477f6c0b053ded6d0852c1786f86622cf29bb74db5689bb4ae69b675"),
    ("dna4_k10", cd.N_READS, None, False): ("6c87e35acb295d4873bac10b144b2cb06f61aefb79615109ea18216680fcf9af", None),
    ("aa20_k5", cd.N_READS, None, False): ("c70f67f6e4dd933a7ebaaa372f9af0e63d7167ffdc6acee03970c3983abcc4b6", None),
    ("dna4_k10", cd.N_READS, None, True): ("53c97587a7c1e7c8c5d68ef9a61891bc49578d2f5c4abc997c5c95f4bc6ea60a", None),
    ("aa20_k5", cd.N_READS, None, True): ("b58759dc0adda9978bffd9a44c6ec867c60ee8ef23c7f0581b8a9dcc3dc0dde6", None),
}
PAIRS = {
    "dna4_k10": ("fdd950545e8586a2ffa267732d3df383740d69c23de96616155bc3a9f15efeff", "5dee3ccc854b5011c70f7a4c2642ff7e13d5ce83e03c13f0352e998e46a4a280"),
    "aa20_k5": ("950fe1f060f76407dade6e7aa16b92a4302043bebcfd94b0e5b43e5eb1d7c399", "34791fcfaae1894619e2793fa2d4bb1684081054770a45fdf79c3b927bb56910"),
}
# name -> (what is hashed, the digest)
OTHERS = {
    "repeat_text": (lambda: cd.repeat_text(), "6a8d728e5ef55f7476edbde8bf30440d912fc27da687ccf358fd9868a5ca4133"),
    "repeat_pair": (lambda: cd.repeat_pair(), "a8bea4faf7cb5e9fb3596070d2e2fe7caade3d73b4c8ef30de7ec41fdd6c677b"),
    "copies_text": (lambda: (cd.copies_text(),), "26ce1119c1dbd7968fe048b18a56b1af2ea373f8e1f32d4df215ba20145b2ebf"),
    "planted_text": (lambda: cd.planted_text(), "51097522fccb30255af4a2e652d1f1e2c2830a15ff8cdae6e6cc8d8a23d7585b"),
    "pair_text": (lambda: (cd.pair_text(),), "3f09b70ec2d6512c1d4ab21e146c98605717eb5d0c08e2c0f05cd3862efb99a5"),
    "clip_text": (lambda: (cd.clip_text(),), "57633012f83e421253b28e029cef960cacfafc73edb4041726c01b5529743e17"),
    "clip_planted_reads": (lambda: pack(cd.clip_planted_reads()), "b705ed2e1e7427e0d7b76767468f3bfa24666733c55ae4f0fe8c7ed82cb95edb"),
    "table_reads": (lambda: pack(cd.table_reads()), "4c62c5126c7ef2848d9481f22110b9f66e02f06328592af45a233165f9c81a13"),
    "realign_batch": (lambda: pack(cd.realign_batch()), "5cc7df254849091c619c30751ec4a0df63d63df98d876283bed7c5fad108af14"),
    "boundary_reads": (lambda: pack(cd.boundary_reads()[0]) + pack(cd.boundary_reads()[1]), "08010428a9733f19b9a2a43f3d2f76b67ea4c52a3cb00304ee474342d7100146"),
    "supp_text": (lambda: (cd.supp_text(),), "583a944e3e4ce6d9458c2eedb4b54016fd2def48913be5d6c8fcb4591a97b6ed"),
    "units": (lambda: cd.units(), "38d591f2c65bb009425fae2268175c7504f1699a45ab81ddbabe9df53239e932"),
    "supp_planted_reads": (lambda: pack(cd.supp_planted_reads()), "c4b354d356d9095e4db280d8f54cb372a4c9886627acecdba8159b6d0ec5d839"),
    "public_c": (lambda: fd.public_c(), "3d84a3db17d83d5a2d9de15a87b96e309880848170bcb8c9fceb39ce05a84512"),
    "pairs_d": (lambda: fd.pairs_d(), "ca3f13e9c4193f1e35d7d7f36abdc2a60eecdcc906fa001a6a19935882088665"),
}
# layout -> (the text, reads_a, reads_b or None)
LAYOUTS = {
    "dna4_k6_s3": ("8c07047a51d16fe0cd35f89a748a78f546d6dc153196c1ee3855341adbf920c4", "d7259eb391831b7cdcb3b9afaa6cfed12b2e4d5770a93bc2055a0f4765d43fd8", None),
    "dna4_k6_s4": ("eb03e39a2fd8da2fd987222069e8f185d3ebd5bd8054ecf987d7a9e508812cb2", "7861aa547ecf4a70f0cd54ec3791524453fe6037f7f849a2eeef9c0deca57315",
                   "d1980751d5fc0f00aac8afdb4acf321b96696234eafa1b4702934e5fd713fb76"),
    "dna4_k6_s5": ("2753287e69a33a7a7303269c8ce3925e5e39bda08341478f8db31dba1fa51557", "ca37283b795006e306deeaf26a5d6466f5d1da68d56924243fbaa3d314aa16f5",
                   "40d73280e8fafe6f1a9bbcff9c5e8b3a0307639dae455232e961160e0dfb591b"),
    "dna4_k6_plain": ("2120d3c760a2fd34ba7b1a424e5c0b5eadfc5d822addd58677cf7abf5193100f", "87a9a8de779673f93ea42ed6b9512703b5374df8ce50b16e50be16b2fa9d1f49", None),
    "dna4_k6_atab": ("d1455aa53c8ba2c8e986f97faa6acb368452b42b38dfd5f5ead9520253b90cde", "0f5ab623e20539906eb1d7a242a271ff0df59a1e3db16fe4f1c547ec5524d306", None),
    "dna5_k5_s4": ("08d9d3f608b07367750e861369dfa5b86c6151a41e446b88e7193e7c8aad0125", "178ccb41293807a0ea264f3f3af6814b40abb67ca7f91c4df478b6501ecc09b9", None),
}
INTERNAL_C = {
    4095: "afcf29404b6ad324584f2137fdef820d49ad3284dbbd5c734fa9a4c977706588",
    4096: "896ee1d1aac3016bf2351a95b9134b972c309d3725fb5e4f5ed4f99f6f154d79",
    4097: "2377f27c3672ad9caa9d31d1c665d9880def172983b649e2652db70068fdbcb4",
    4098: "05edd9d92be14566466df427266c6de3b785c701a3c83018b9883edd5c890a70",
    8193: "515e253d3580b568c1acf139de1ad1740ca838bd09910ccaeb75c0ad33f48020",
}


@pytest.mark.parametrize("sigma,n", sorted(TEXTS))
def test_texts(sigma, n):
    assert digest(cd.text_of(sigma, n)) == TEXTS[(sigma, n)]
    assert not cd.text_of(sigma, n).flags.writeable


def test_every_workload_of_the_tests_is_pinned():
    assert {k[0] for k in READS if k[1] is None} == set(cd.READ_WORKLOADS) and set(PAIRS) == set(cd.PAIR_WORKLOADS) == set(cd.PAIR_FLOORS)
    assert set(cd.RESCUE_FLOORS) == set(PAIRS) and {k[0] for k in cd.STRAND_FLOORS} <= {k[0] for k in READS if k[3]}
    assert set(LAYOUTS) == set(fd.LAYOUTS) and sorted(INTERNAL_C) == sorted(fd.C_DIRECT + tuple(2 * x for x in fd.C_PUBLIC))
    assert cd.N_READS == 600 and cd.N_PAIRS == 300


@pytest.mark.parametrize("name,n_reads,meta,reverse_odd", sorted(READS, key=repr))
def test_single_reads(name, n_reads, meta, reverse_odd):
    got = cd.reads_of(name, n_reads, meta, reverse_odd)
    want, want_meta = READS[(name, n_reads, meta, reverse_odd)]
    assert digest(got[0], got[1]) == want
    assert len(got) == (3 if meta else 2) and got[1].size - 1 == (n_reads or cd.READ_WORKLOADS[name][3])
    if meta:
        assert digest_of_meta(got[2]) == want_meta and len(got[2][0]) == (5 if meta == "bad" else 4)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_pairs(name):
    assert (digest(*cd.pairs_of(name)), digest(*cd.rescue_pairs_of(name))) == PAIRS[name]


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_texts_and_planted_reads(name):
    make, want = OTHERS[name]
    assert digest(*make()) == want


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_front_layouts(name):
    text, a, b = LAYOUTS[name]
    assert digest(fd.layout_text(name)) == text and digest(*fd.reads_a(name)) == a
    if b is not None:
        assert digest(*fd.reads_b(name)) == b


@pytest.mark.parametrize("nr2", sorted(INTERNAL_C))
def test_front_internal_reads(nr2):
    assert digest(*fd.internal_c(nr2)) == INTERNAL_C[nr2]
