"""The exact text of every refusal of StreamPool, NativeStreamPool and NativeRatePool that is reached before a device is needed: one
table of (call, exception type, message), each held to str(exception) == message.  The order of a call's refusals shows in the cases
that are wrong in two ways at once.  No compute and no device here: the model is a BSRNN() that never gets a context;
tests/test_gpu_stream_refusals.py holds the refusals that need a stream."""
import os

import pytest

from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
RESAMPLE = "resample: cannot convert 1 samples from %s to 44100 Hz (rates >= 1, reduced max(up, down) <= 1024, n >= 1)"
OWN_RATE_STEP = "%s.step: session 0 has a sample rate of its own (48000 Hz): its audio does not come in whole hops, use feed()"
OWN_RATE_EXPORT = "%s.export: session 0 has a sample rate of its own (48000 Hz); the resamplers' carries do not move with a session"
STRIDES = ("NativeStreamPool.feed: session 1: strides %s; the chunk goes by pointer and row stride, so samples of a row must be adjacent and "
           "rows must not overlap")
NO_RATES = ("NativeStreamPool.open: sample_rate %r: the native pool serves sessions at the model's 44100 Hz; sessions with a rate of their own "
            "are StreamPool(rates=...)'s")


@pytest.fixture(scope="module")
def world():
    """One model without a device and a full pool of each kind, 3 slots x 2 rows: session 0 at 48 kHz where the pool has rates, sessions
    1 and 2 at the model's rate."""
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from speechseparation_amd.bsrnn import BSRNN, NativeRatePool, NativeStreamPool, StreamPool
    m = BSRNN()
    sp = StreamPool(m, 3, 2, rates=(16000, 48000))
    plain = StreamPool(m, 2, 2)
    nat = NativeStreamPool(m, 3, rows_per_session=2, max_hops=3)
    rat = NativeRatePool(m, 3, rows_per_session=2, max_hops=3, rates=(16000, 48000), max_block=4800)
    assert [sp.open(sample_rate=48000), sp.open(), sp.open(sample_rate=44100)] == [0, 1, 2]
    assert [nat.open(), nat.open(), nat.open(sample_rate=44100)] == [0, 1, 2]
    assert [rat.open(sample_rate=48000), rat.open(), rat.open(sample_rate=44100)] == [0, 1, 2]
    return m, sp, plain, nat, rat


def _cases(m, sp, plain, nat, rat):
    import torch
    from speechseparation_amd.bsrnn import NativeRatePool, NativeStreamPool, StreamPool
    V, K = ValueError, KeyError
    nf = 2 * 2048 + 8 * len(m.band_widths) * 64
    blob = torch.zeros(nf)
    some, hop, wide = torch.zeros((2, 700)), torch.zeros((2, 1024)), torch.zeros((2, 2048))
    cases = []

    def case(call, exc, message):
        cases.append((call, exc, message))

    # ---- the constructors: rates first, then (NativeRatePool) max_block, then the ints in the order of the parameters, then the rows
    for cls, name in ((StreamPool, "StreamPool"), (NativeStreamPool, "NativeStreamPool")):
        case(lambda cls=cls: cls(m, 0), V, "%s: slots must be a positive int, got 0" % name)
        case(lambda cls=cls: cls(m, True), V, "%s: slots must be a positive int, got True" % name)
        case(lambda cls=cls: cls(m, 2.5), V, "%s: slots must be a positive int, got 2.5" % name)
        case(lambda cls=cls: cls(m, "2"), V, "%s: slots must be a positive int, got '2'" % name)
        case(lambda cls=cls: cls(m, 0, rows_per_session=0), V, "%s: slots must be a positive int, got 0" % name)
        case(lambda cls=cls: cls(m, 2, rows_per_session=0), V, "%s: rows_per_session must be a positive int, got 0" % name)
        case(lambda cls=cls: cls(m, 2, rows_per_session=-1), V, "%s: rows_per_session must be a positive int, got -1" % name)
        case(lambda cls=cls: cls(m, 1025, rows_per_session=2), V, "%s: 1025 slots x 2 rows is more than the 2048 rows a rows call takes" % name)
    case(lambda: NativeStreamPool(m, 2, max_hops=0), V, "NativeStreamPool: max_hops must be a positive int, got 0")
    case(lambda: NativeStreamPool(m, 2, max_hops=2.0), V, "NativeStreamPool: max_hops must be a positive int, got 2.0")
    case(lambda: NativeStreamPool(m, 2, max_hops=256), V, "NativeStreamPool: max_hops = 256, a hops call takes at most 255")
    case(lambda: NativeStreamPool(m, 2049, max_hops=256), V, "NativeStreamPool: 2049 slots x 1 rows is more than the 2048 rows a rows call takes")
    for make in (lambda **kw: StreamPool(m, 0, 2, **kw), lambda **kw: NativeRatePool(m, 0, max_block=0, **kw)):      # (the rates come first)
        case(lambda make=make: make(rates=48000), V, "StreamPool: rates must be a tuple of sample rates, got int")
        case(lambda make=make: make(rates=()), V, "StreamPool: 0 rates, a pool takes 1 to 16")
        case(lambda make=make: make(rates=tuple(range(8000, 8017))), V, "StreamPool: 17 rates, a pool takes 1 to 16")
        case(lambda make=make: make(rates=(16000, 48000.0)), V, "StreamPool: a rate must be an int, got 48000.0")
        case(lambda make=make: make(rates=(True,)), V, "StreamPool: a rate must be an int, got True")
        case(lambda make=make: make(rates=("48000",)), V, "StreamPool: a rate must be an int, got '48000'")
        case(lambda make=make: make(rates=(16000, 0)), V, RESAMPLE % 0)
        case(lambda make=make: make(rates=(48001,)), V, RESAMPLE % 48001)                       # 48001 / 44100 does not reduce
    case(lambda: NativeRatePool(m, 0, rates=None), V, "NativeRatePool: rates must be a tuple of sample rates, got None (a pool without is NativeStreamPool)")
    for bad in (0, 2.5, True, (1 << 24) + 1):
        case(lambda bad=bad: NativeRatePool(m, 0, max_block=bad), V, "NativeRatePool: max_block must be an int in [1, 2^24], got %r" % (bad,))
    case(lambda: NativeRatePool(m, 0), V, "NativeStreamPool: slots must be a positive int, got 0")
    case(lambda: NativeRatePool(m, 2, rows_per_session=0), V, "NativeStreamPool: rows_per_session must be a positive int, got 0")
    case(lambda: NativeRatePool(m, 2, max_hops=0), V, "NativeStreamPool: max_hops must be a positive int, got 0")
    case(lambda: NativeRatePool(m, 2, max_hops=256), V, "NativeStreamPool: max_hops = 256, a hops call takes at most 255")
    case(lambda: NativeRatePool(m, 1025, 2), V, "NativeStreamPool: 1025 slots x 2 rows is more than the 2048 rows a rows call takes")

    # ---- open: the rate before the slots
    case(lambda: sp.open(sample_rate=8000), V, "StreamPool.open: sample_rate 8000 is not one of the pool's rates (16000, 48000)")
    case(lambda: sp.open(sample_rate="48000"), V, "StreamPool.open: sample_rate '48000' is not one of the pool's rates (16000, 48000)")
    case(lambda: plain.open(sample_rate=48000), V, "StreamPool.open: sample_rate 48000 is not one of the pool's rates None")
    case(lambda: sp.open(), V, "StreamPool: all 3 slots are in use")
    case(lambda: sp.open(sample_rate=16000), V, "StreamPool: all 3 slots are in use")
    case(lambda: nat.open(sample_rate=48000), V, NO_RATES % 48000)
    case(lambda: nat.open(sample_rate="44100"), V, NO_RATES % "44100")
    case(lambda: nat.open(), V, "NativeStreamPool: all 3 slots are in use")
    case(lambda: nat.open(sample_rate=44100), V, "NativeStreamPool: all 3 slots are in use")
    case(lambda: rat.open(sample_rate=22050), V, "NativeRatePool.open: sample_rate 22050 is not one of the pool's rates (16000, 48000)")
    case(lambda: rat.open(sample_rate="48000"), V, "NativeRatePool.open: sample_rate '48000' is not one of the pool's rates (16000, 48000)")
    case(lambda: rat.open(), V, "NativeRatePool: all 3 slots are in use")
    case(lambda: rat.open(sample_rate=16000), V, "NativeRatePool: all 3 slots are in use")

    # ---- feed and step, what the three pools share: a dict, known sessions, [rows, n] tensors; then the mix.  A NativeRatePool refuses
    # ---- with the inherited code, under NativeStreamPool's name
    for pool, name in ((sp, "StreamPool"), (nat, "NativeStreamPool"), (rat, "NativeStreamPool")):
        for call, what, shape in ((pool.feed, "feed", "n"), (pool.step, "step", "L*1024")):
            who = "%s.%s" % (name, what)
            need = "%s: session 1 needs a tensor [2, %s], got " % (who, shape)
            case(lambda call=call: call([hop]), V, "%s: chunks must be a dict {session id: tensor}, got list" % who)
            case(lambda call=call: call(hop), V, "%s: chunks must be a dict {session id: tensor}, got Tensor" % who)
            case(lambda call=call: call({77: hop}), K, "77")
            case(lambda call=call: call({77: "chunk"}), K, "77")
            case(lambda call=call: call({1: hop, 77: hop}), K, "77")
            case(lambda call=call: call({1: torch.zeros((1, 1024))}), V, need + "(1, 1024)")
            case(lambda call=call: call({1: torch.zeros((3, 1024))}), V, need + "(3, 1024)")
            case(lambda call=call: call({1: torch.zeros(1024)}), V, need + "(1024,)")
            case(lambda call=call: call({1: torch.zeros((1, 2, 1024))}), V, need + "(1, 2, 1024)")
            case(lambda call=call: call({1: "chunk"}), V, need + "str")
            case(lambda call=call: call({1: hop.numpy()}), V, need + "ndarray")
            case(lambda call=call: call({1: hop, 2: None}), V, need.replace("session 1", "session 2") + "NoneType")
            case(lambda call=call: call({1: hop}, mix="wet"), V, "%s: mix must be None, a float or a dict {session id: float}, got str" % who)
            case(lambda call=call: call({1: hop}, mix=True), V, "%s: mix must be None, a float or a dict {session id: float}, got bool" % who)
            case(lambda call=call: call({1: hop}, mix=[0.5]), V, "%s: mix must be None, a float or a dict {session id: float}, got list" % who)
            case(lambda call=call: call({1: hop}, mix=torch.ones(6)), V,
                 "%s: mix must be None, a float or a dict {session id: float}, got Tensor" % who)
            case(lambda call=call: call({1: hop}, mix={1: "wet"}), V, "%s: mix of session 1 must be a float, got str" % who)
            case(lambda call=call: call({1: hop}, mix={2: 0.5, 1: False}), V, "%s: mix of session 1 must be a float, got bool" % who)
            case(lambda call=call: call({1: hop}, mix={77: 0.5}), K, "77")
            case(lambda call=call: call({1: hop}, mix={77: "wet"}), K, "77")
            case(lambda call=call: call({}, mix="wet"), V, "%s: mix must be None, a float or a dict {session id: float}, got str" % who)
            case(lambda call=call: call({1: "chunk"}, mix="wet"), V, need + "str")                # (the chunks before the mix)
        # step: whole hops, one L for all
        who = "%s.step" % name
        case(lambda pool=pool: pool.step({1: some}), V, "%s: session 1 holds 700 samples per row, need whole hops of 1024" % who)
        case(lambda pool=pool: pool.step({1: torch.zeros((2, 0))}), V, "%s: session 1 holds 0 samples per row, need whole hops of 1024" % who)
        case(lambda pool=pool: pool.step({1: hop, 2: wide}), V, "%s: session 2 holds 2048 samples per row, the others 1024 (one L per step)" % who)
        case(lambda pool=pool: pool.step({2: wide, 1: hop}), V, "%s: session 1 holds 1024 samples per row, the others 2048 (one L per step)" % who)
        case(lambda pool=pool: pool.step({1: hop, 2: some}), V, "%s: session 2 holds 700 samples per row, need whole hops of 1024" % who)
        case(lambda pool=pool: pool.step({1: some, 77: hop}), V, "%s: session 1 holds 700 samples per row, need whole hops of 1024" % who)
        case(lambda pool=pool: pool.step({1: some}, mix="wet"), V, "%s: session 1 holds 700 samples per row, need whole hops of 1024" % who)

    # ---- the native pools' feed: chunks that cannot go by pointer
    for pool in (nat, rat):
        case(lambda pool=pool: pool.feed({1: some.double()}), V,
             "NativeStreamPool.feed: session 1 needs float32 samples, got torch.float64 (the chunk goes by pointer)")
        case(lambda pool=pool: pool.feed({1: some.to(torch.int32)}), V,
             "NativeStreamPool.feed: session 1 needs float32 samples, got torch.int32 (the chunk goes by pointer)")
        case(lambda pool=pool: pool.feed({1: wide[:, ::2]}), V, STRIDES % "(2048, 2)")
        case(lambda pool=pool: pool.feed({1: torch.zeros((700, 2)).t()}), V, STRIDES % "(1, 2)")
        case(lambda pool=pool: pool.feed({1: torch.zeros((1, 700)).expand(2, 700)}), V, STRIDES % "(0, 1)")
        case(lambda pool=pool: pool.feed({1: some.double()}, mix="wet"), V,
             "NativeStreamPool.feed: session 1 needs float32 samples, got torch.float64 (the chunk goes by pointer)")
        # a step is a feed behind its own checks
        case(lambda pool=pool: pool.step({1: hop.double()}), V,
             "NativeStreamPool.feed: session 1 needs float32 samples, got torch.float64 (the chunk goes by pointer)")
        case(lambda pool=pool: pool.step({1: torch.zeros((2, 2048))[:, ::2]}), V, STRIDES % "(2048, 2)")
        if torch.cuda.is_available():
            case(lambda pool=pool: pool.feed({1: some, 2: some.cuda()}), V, "NativeStreamPool.feed: CUDA and CPU chunks in one call; a feed takes one kind")
            case(lambda pool=pool: pool.feed({1: some.cuda(), 2: some}), V, "NativeStreamPool.feed: CUDA and CPU chunks in one call; a feed takes one kind")

    # ---- sessions with a sample rate of their own
    case(lambda: sp.step({0: hop}), V, OWN_RATE_STEP % "StreamPool")
    case(lambda: sp.step({1: hop, 0: hop}), V, OWN_RATE_STEP % "StreamPool")
    case(lambda: sp.step({0: some}), V, "StreamPool.step: session 0 holds 700 samples per row, need whole hops of 1024")     # (the shape first)
    case(lambda: sp.step({0: hop, 1: "chunk"}), V, OWN_RATE_STEP % "StreamPool")                 # (session by session)
    case(lambda: rat.step({0: hop}), V, OWN_RATE_STEP % "NativeRatePool")
    case(lambda: rat.step({1: hop, 0: hop}), V, OWN_RATE_STEP % "NativeRatePool")
    case(lambda: rat.step({1: "chunk", 0: some}), V, OWN_RATE_STEP % "NativeRatePool")           # (before every other check of the chunks)
    case(lambda: rat.step({0: hop, 77: hop}), V, OWN_RATE_STEP % "NativeRatePool")
    case(lambda: rat.feed({0: torch.zeros((2, 4801))}), V,
         "NativeRatePool.feed: session 0 brings 4801 samples per row, the pool was created for max_block = 4800")
    case(lambda: rat.feed({1: some, 0: torch.zeros((2, 4801))}), V,
         "NativeRatePool.feed: session 0 brings 4801 samples per row, the pool was created for max_block = 4800")
    cpu_chunk = ("NativeRatePool.feed: session 0 has a sample rate of its own (48000 Hz) and brings a CPU chunk; the host form serves sessions at "
                 "the model's rate")
    case(lambda: rat.feed({0: some}), V, cpu_chunk)
    case(lambda: rat.feed({1: some, 0: some}), V, cpu_chunk)
    case(lambda: rat.feed({77: some, 0: some}), V, cpu_chunk)                                    # (before the sessions are looked up)
    case(lambda: rat.feed({0: torch.zeros((3, 700))}), V, cpu_chunk)                             # (and before the rows are counted)
    case(lambda: rat.feed({0: torch.zeros(700)}), V, "NativeStreamPool.feed: session 0 needs a tensor [2, n], got (700,)")
    case(lambda: sp.export(0), V, OWN_RATE_EXPORT % "StreamPool")
    case(lambda: rat.export(0), V, OWN_RATE_EXPORT % "NativeRatePool")

    # ---- drain's mix: None or a float
    for pool, name in ((sp, "StreamPool"), (rat, "NativeRatePool")):
        for bad in ("wet", True, {0: 0.5}, [0.5]):
            case(lambda pool=pool, bad=bad: pool.drain(0, mix=bad), V, "%s.drain: mix must be None or a float, got %s" % (name, type(bad).__name__))
        case(lambda pool=pool: pool.drain(1, mix="wet"), V, "%s.drain: mix must be None or a float, got str" % name)
        case(lambda pool=pool: pool.drain(77, mix="wet"), K, "77")
        case(lambda pool=pool: pool.drain(77), K, "77")

    # ---- adopt: the blobs, then (native) what waits, then the slots
    for pool, name in ((sp, "StreamPool"), (nat, "NativeStreamPool"), (rat, "NativeStreamPool")):
        need = "%s.adopt: need 2 blobs of %d floats each" % (name, nf)
        case(lambda pool=pool: pool.adopt([torch.zeros(5)] * 2), V, need)
        case(lambda pool=pool: pool.adopt([blob]), V, need)
        case(lambda pool=pool: pool.adopt([blob] * 3), V, need)
        case(lambda pool=pool: pool.adopt([blob, blob.view(1, -1)]), V, need)
        case(lambda pool=pool: pool.adopt([blob, blob.numpy()]), V, need)
        case(lambda pool=pool: pool.adopt([]), V, need)
    case(lambda: sp.adopt([blob, blob]), V, "StreamPool: all 3 slots are in use")
    for pool, full in ((nat, "NativeStreamPool: all 3 slots are in use"), (rat, "NativeStreamPool: all 3 slots are in use")):
        need = "NativeStreamPool.adopt: pending must be a tensor [2, n] with n < 1024, got "
        case(lambda pool=pool: pool.adopt([blob, blob], hop), V, need + "(2, 1024)")
        case(lambda pool=pool: pool.adopt([blob, blob], torch.zeros((1, 10))), V, need + "(1, 10)")
        case(lambda pool=pool: pool.adopt([blob, blob], torch.zeros(10)), V, need + "(10,)")
        case(lambda pool=pool: pool.adopt([blob, blob], "fifo"), V, need + "str")
        case(lambda pool=pool: pool.adopt([blob], hop), V, "NativeStreamPool.adopt: need 2 blobs of %d floats each" % nf)
        case(lambda pool=pool, full=full: pool.adopt([blob, blob]), V, full)
        case(lambda pool=pool, full=full: pool.adopt([blob, blob], some), V, full)
        case(lambda pool=pool, full=full: pool.adopt([blob, blob], torch.zeros((2, 0))), V, full)

    # ---- a session nobody has
    for pool in (sp, plain, nat, rat):
        for call in (pool.close, pool.pending, pool.export) + ((pool.rate_of,) if hasattr(pool, "rate_of") else ()):
            case(lambda call=call: call(77), K, "77")
            case(lambda call=call: call("a"), K, "'a'")
    return cases


def test_every_refusal_before_a_device_has_its_exact_text(world):
    m, sp, plain, nat, rat = world
    cases = _cases(*world)
    assert len(cases) > 300
    for i, (call, exc, message) in enumerate(cases):
        with pytest.raises(exc) as excinfo:
            call()
        assert type(excinfo.value) is exc, (i, message, type(excinfo.value))
        assert str(excinfo.value) == message, (i, str(excinfo.value), message)
    # nothing was taken, nothing was made
    assert sp.sessions() == [0, 1, 2] and nat.sessions() == [0, 1, 2] and rat.sessions() == [0, 1, 2] and plain.sessions() == []
    assert [sp.rate_of(s) for s in (0, 1, 2)] == [48000, 44100, 44100] == [rat.rate_of(s) for s in (0, 1, 2)]
    assert sp._free == [] and nat._free == [] and rat._free == [] and plain._free == [0, 1]
    assert sp._st is None and plain._st is None and nat._h is None and rat._h is None
    assert m._ctx is None
