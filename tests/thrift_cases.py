"""Hand-built thriftrw protocol.Binary history blobs for the device decoder's tests
(tests/test_ingest_wire.py): what the synthetic encoder (csrc/thrift_enc.cpp) never
writes.  CPU only, no GPU and no libcdr.

A blob is a small tree: a struct is ``St(name, [F(type, id, value), ...])``; a field's
value is a Python int / float (fixed types), bytes (string), an ``St``, ``Raw(bytes)`` (a
pre-encoded value) or, for containers, ``Lst(elem type, [values])`` /
``Mp(key type, value type, [(key, value)])``.  ``value`` / ``blob`` write it with the writer of
oracle/thrift_binary.py.  Mutators walk the tree, so a case can name the struct it
changes (``St.name``).

A case is a tuple (name, blob bytes, expected blob status, "strict" | "by-string").
"""
from __future__ import annotations

import struct

from cadence_amd import abi
from oracle import thrift_binary as TB
from oracle import thrift_decode as TD
from oracle.thrift_binary import field, struct_

T_BOOL, T_BYTE, T_DOUBLE, T_I16, T_I32, T_I64, T_STRING, T_STRUCT, T_MAP, T_SET, T_LIST = (
    TD.T_BOOL, TD.T_BYTE, TD.T_DOUBLE, TD.T_I16, TD.T_I32, TD.T_I64, TD.T_STRING, TD.T_STRUCT, TD.T_MAP, TD.T_SET,
    TD.T_LIST)
STRICT, BY_STRING = "strict", "by-string"
OK = TD.DEC_OK


# ------------------------------------------------------------------ the tree and its writer
class St:
    def __init__(self, name, fields):
        self.name, self.fields = name, list(fields)


class F:
    def __init__(self, t, fid, v):
        self.t, self.fid, self.v = t, fid, v


class Lst:  # a list (or, with T_SET on the field, a set) value
    def __init__(self, et, items):
        self.et, self.items = et, list(items)


class Mp:
    def __init__(self, kt, vt, pairs):
        self.kt, self.vt, self.pairs = kt, vt, list(pairs)


class Raw:
    def __init__(self, b):
        self.b = bytes(b)


_FIXED = {T_BOOL: ">b", T_BYTE: ">b", T_I16: ">h", T_I32: ">i", T_I64: ">q", T_DOUBLE: ">d"}


def value(t, v) -> bytes:
    """The wire bytes of one value of wire type t."""
    if isinstance(v, Raw):
        return v.b
    if t in _FIXED:
        return struct.pack(_FIXED[t], v)
    if t == T_STRING:
        return struct.pack(">i", len(v)) + bytes(v)
    if t == T_STRUCT:
        return struct_([field(f.t, f.fid, value(f.t, f.v)) for f in v.fields])
    if t in (T_LIST, T_SET):
        return struct.pack(">bi", v.et, len(v.items)) + b"".join(value(v.et, x) for x in v.items)
    if t == T_MAP:
        return struct.pack(">bbi", v.kt, v.vt, len(v.pairs)) + b"".join(
            value(v.kt, k) + value(v.vt, x) for k, x in v.pairs)
    raise ValueError(t)


def s(fid, b):
    return F(T_STRING, fid, b)


def i32(fid, v):
    return F(T_I32, fid, v)


def i64(fid, v):
    return F(T_I64, fid, v)


def boolean(fid, v):
    return F(T_BOOL, fid, 1 if v else 0)


def sub(fid, name, fields):
    return F(T_STRUCT, fid, St(name, fields))


def lst(fid, et, items):
    return F(T_LIST, fid, Lst(et, items))


def mp(fid, kt, vt, pairs):
    return F(T_MAP, fid, Mp(kt, vt, pairs))


def blob(history: St) -> bytes:
    """Codec preamble + the History struct."""
    return TB.PREAMBLE + value(T_STRUCT, history)


def history(events, extra=()):
    return St("History", [lst(10, T_STRUCT, events)] + list(extra))


# ------------------------------------------------------------------ well-formed events
# HistoryEvent field of each attribute struct -> its event type (shared.thrift:868-916)
ATTR_TYPE = {
    40: "WorkflowExecutionStarted", 50: "WorkflowExecutionCompleted", 80: "DecisionTaskScheduled", 90: "DecisionTaskStarted",
    100: "DecisionTaskCompleted", 110: "DecisionTaskTimedOut", 120: "DecisionTaskFailed",
    130: "ActivityTaskScheduled", 140: "ActivityTaskStarted", 150: "ActivityTaskCompleted",
    160: "ActivityTaskFailed", 170: "ActivityTaskTimedOut", 180: "TimerStarted", 190: "TimerFired",
    200: "ActivityTaskCancelRequested", 210: "RequestCancelActivityTaskFailed", 220: "ActivityTaskCanceled",
    230: "TimerCanceled", 240: "CancelTimerFailed", 300: "RequestCancelExternalWorkflowExecutionInitiated",
    310: "RequestCancelExternalWorkflowExecutionFailed", 320: "ExternalWorkflowExecutionCancelRequested",
    330: "WorkflowExecutionContinuedAsNew", 340: "StartChildWorkflowExecutionInitiated",
    350: "StartChildWorkflowExecutionFailed", 360: "ChildWorkflowExecutionStarted",
    370: "ChildWorkflowExecutionCompleted", 380: "ChildWorkflowExecutionFailed",
    390: "ChildWorkflowExecutionCanceled", 400: "ChildWorkflowExecutionTimedOut",
    410: "ChildWorkflowExecutionTerminated", 420: "SignalExternalWorkflowExecutionInitiated",
    430: "SignalExternalWorkflowExecutionFailed", 440: "ExternalWorkflowExecutionSignaled",
    450: "UpsertWorkflowSearchAttributes",
}


def event(eid, attr, fields, version=7, task_id=None):
    """HistoryEvent{10 eventId, 20 timestamp, 30 eventType, 35 version, 36 taskId, attr}."""
    return St("HistoryEvent", [
        i64(10, eid), i64(20, 1_600_000_000_000_000_000 + eid), i32(30, abi.EV[ATTR_TYPE[attr]]), i64(35, version),
        i64(36, 5000 + eid if task_id is None else task_id), sub(attr, "attr%d" % attr, fields)])


def name(fid, kind, n):
    return sub(fid, kind, [s(10, n)])


def execution(fid, wid, rid):
    return sub(fid, "WorkflowExecution", [s(10, wid), s(20, rid)])


def retry_policy(fid, reasons=(b"bad", b"worse")):
    f = [i32(10, 2), F(T_DOUBLE, 20, 1.5), i32(30, 60), i32(40, 5)]
    if reasons is not None:
        f.append(lst(50, T_STRING, list(reasons)))
    return sub(fid, "RetryPolicy", f + [i32(60, 600)])


def search_attributes(fid, pairs):
    return sub(fid, "SearchAttributes", [mp(10, T_STRING, T_STRING, pairs)])


def reset_point(cks, run, k):
    return St("ResetPointInfo", [s(10, cks), s(20, run), i64(30, 4 + k), i64(40, 10**18 + k), i64(50, 2 * 10**18 + k),
                                 boolean(60, k % 2 == 0)])


def reset_points(fid, pts):
    return sub(fid, "ResetPoints", [lst(10, T_STRUCT, pts)])


def memo(fid, pairs=((b"mk", b"mv"),)):
    return sub(fid, "Memo", [mp(10, T_STRING, T_STRING, pairs)])


def started(eid, tag=b"", full=True, sa=((b"k1", b"v1"), (b"k2", b"v2")), n_rp=2):
    """WorkflowExecutionStarted with everything the record keeps (`tag` makes its strings
    distinct from another event's)."""
    f = [name(10, "WorkflowType", b"wt" + tag), s(12, b"pdom"), execution(14, b"pw" + tag, b"pr" + tag), i64(16, 3),
         name(20, "TaskList", b"tl" + tag), s(30, b"input-not-kept"), i32(40, 3600), i32(50, 10), s(54, b"crun" + tag),
         i32(55, 2)]
    if full:
        f += [retry_policy(70), i32(80, 1), i64(90, 1_700_000_000), s(100, b"* * * * *"), i32(110, 30), memo(120)]
    if sa is not None:
        f.append(search_attributes(121, [(k + tag, v + tag) for k, v in sa]))
    if n_rp is not None:
        f.append(reset_points(130, [reset_point(b"ck%d" % k + tag, b"rr%d" % k + tag, k) for k in range(n_rp)]))
    return event(eid, 40, f)


def decision_scheduled(eid):
    return event(eid, 80, [name(10, "TaskList", b"tl"), i32(20, 10), i64(30, 1)])


def decision_started(eid):
    return event(eid, 90, [i64(10, eid - 1), s(20, b"identity-not-kept"), s(30, b"req-d")])


def decision_completed(eid):
    return event(eid, 100, [s(10, b"ctx-not-kept"), i64(20, eid - 2), i64(30, eid - 1), s(50, b"cksum")])


def decision_timed_out(eid):
    return event(eid, 110, [i64(10, eid - 2), i64(20, eid - 1), i32(30, 1)])


def activity_scheduled(eid, domain=None):
    f = [s(10, b"act-1")]
    if domain is not None:
        f.append(s(25, domain))
    return event(eid, 130, f + [name(30, "TaskList", b"atl"), i32(45, 100), i32(50, 20), i32(55, 80), i32(60, 5),
                                retry_policy(110, reasons=None)])


def activity_started(eid):
    return event(eid, 140, [i64(10, eid - 1), s(30, b"req-a"), i32(40, 2)])


def activity_completed(eid):
    return event(eid, 150, [s(10, b"result-not-kept"), i64(20, eid - 2), i64(30, eid - 1)])


def activity_timed_out(eid):
    return event(eid, 170, [i64(10, eid - 2), i64(20, eid - 1), i32(30, 2)])


def activity_cancel_requested(eid):
    return event(eid, 200, [s(10, b"act-1"), i64(20, 4)])


def timer_started(eid):
    return event(eid, 180, [s(10, b"timer-1"), i64(20, 30), i64(30, 4)])


def timer_fired(eid):
    return event(eid, 190, [s(10, b"timer-1"), i64(20, eid - 1)])


def child_initiated(eid, domain=b"cdom"):
    return event(eid, 340, [s(10, domain), s(20, b"child-wf"), name(30, "WorkflowType", b"cwt"), s(50, b"cin"),
                            i32(81, 1), s(90, b"cctl")])


def signal_initiated(eid, domain=b"sdom", control=b"sctl"):
    return event(eid, 420, [s(20, domain), execution(30, b"sw", b"sr"), s(40, b"sig"), s(50, b"sin"), s(60, control),
                            boolean(70, True)])


def cancel_initiated(eid, domain=b"xdom", control=b"xctl"):
    return event(eid, 300, [s(20, domain), execution(30, b"xw", b"xr"), s(40, control), boolean(50, True)])


def child_completed(eid):  # a ref type with a WorkflowExecution
    return event(eid, 370, [s(10, b"res-not-kept"), s(20, b"cdom"), execution(30, b"child-wf", b"child-run"),
                            name(40, "WorkflowType", b"cwt"), i64(50, 3), i64(60, 4)])


def child_start_failed(eid):  # a ref type without one
    return event(eid, 350, [s(10, b"cdom"), s(20, b"child-wf"), i64(60, 3)])


def external_signaled(eid):
    return event(eid, 440, [i64(10, 3), s(20, b"sdom"), execution(30, b"sw", b"sr")])


def continued_as_new(eid):
    return event(eid, 330, [s(10, b"new-run"), name(20, "WorkflowType", b"wt")])


def upsert(eid, pairs=((b"k1", b"v9"), (b"k3", b"v3"))):
    return event(eid, 450, [i64(10, eid - 1), search_attributes(20, list(pairs))])


def completed(eid):  # an attribute struct the record form does not keep
    return event(eid, 50, [s(10, b"done"), i64(20, eid - 1)])


FAMILIES = [  # one well-formed event of each attribute family the decoder keeps
    started, decision_scheduled, decision_started, decision_completed, decision_timed_out, activity_scheduled,
    activity_started, activity_completed, activity_timed_out, activity_cancel_requested, timer_started, timer_fired,
    child_initiated, signal_initiated, cancel_initiated, child_completed, child_start_failed, external_signaled,
    continued_as_new, upsert, completed]


def family_events():
    return [mk(k + 1) for k, mk in enumerate(FAMILIES)]


# ------------------------------------------------------------------ mutators
def structs(root: St, path=()):
    """Every struct of the tree, with the path (field positions / element indices) to it."""
    yield path, root
    for i, f in enumerate(root.fields):
        yield from _structs_in(f.t, f.v, path + (i,))


def _structs_in(t, v, path):
    if isinstance(v, Raw):
        return
    if t == T_STRUCT:
        yield from structs(v, path)
    elif t in (T_LIST, T_SET):
        for j, x in enumerate(v.items):
            yield from _structs_in(v.et, x, path + (j,))
    elif t == T_MAP:
        for j, (k, x) in enumerate(v.pairs):
            yield from _structs_in(v.vt, x, path + (j,))


def copy(x):
    import copy as _c
    return _c.deepcopy(x)


def at(root: St, path) -> St:
    """The struct at `path` (as `structs` reports it)."""
    node, t = root, T_STRUCT
    for step in path:
        if t == T_STRUCT:
            f = node.fields[step]
            node, t = f.v, f.t
            if t in (T_LIST, T_SET):
                et = node.et
            elif t == T_MAP:
                et = node.vt
        elif t in (T_LIST, T_SET):
            node, t = node.items[step], et
        else:
            node, t = node.pairs[step][1], et
    return node


def edited(root: St, path, fn) -> St:
    """A copy of the tree with fn(struct at path) applied."""
    r = copy(root)
    fn(at(r, path))
    return r


# unknown values of every wire type (type, value)
def unknown_values():
    e = St("x", [])
    two = St("x", [i32(1, 5), s(2, b"zz")])
    return [
        ("bool", T_BOOL, 1), ("byte", T_BYTE, 0x7F), ("double", T_DOUBLE, -2.5), ("i16", T_I16, -2), ("i32", T_I32, 1 << 30),
        ("i64", T_I64, -(1 << 62)), ("string0", T_STRING, b""), ("string1", T_STRING, b"u"), ("struct0", T_STRUCT, e),
        ("struct2", T_STRUCT, two), ("list0", T_LIST, Lst(T_I32, [])), ("list2", T_LIST, Lst(T_I32, [1, 2])),
        ("list-of-list", T_LIST, Lst(T_LIST, [Lst(T_I64, [1, 2, 3]), Lst(T_I64, [])])),
        ("list-of-struct", T_LIST, Lst(T_STRUCT, [two, e])), ("set0", T_SET, Lst(T_STRING, [])),
        ("set2", T_SET, Lst(T_I64, [4, 5])), ("map0", T_MAP, Mp(T_STRING, T_I32, [])),
        ("map-of-struct", T_MAP, Mp(T_I32, T_STRUCT, [(1, two), (2, e)])),
        ("map-container-keys", T_MAP, Mp(T_LIST, T_MAP, [(Lst(T_I32, [9]), Mp(T_STRING, T_STRING, [(b"a", b"b")])),
                                                         (Lst(T_I32, []), Mp(T_STRING, T_STRING, []))])),
        ("map-strings", T_MAP, Mp(T_STRING, T_STRING, [(b"p", b"q"), (b"", b"")])),
    ]


# ids no struct the decoder walks knows: next to known ones, far from them, negative; at
# the event level 45 and 455 are struct ids outside 40..450 step 10
UNKNOWN_IDS = [9, 11, 39, 41, 451, 460, -1, -32768, 45, 455, 32767, 1]


def insert_unknown(root: St, path, where, fid, t, v) -> St:
    def fn(st):
        n = len(st.fields)
        pos = {"before": 0, "between": n // 2, "after": n}[where]
        st.fields.insert(pos, F(t, fid, copy(v)))
    return edited(root, path, fn)


def one_event_history(ev):
    return history([ev])


def forward_compat_cases():
    """(a) an unknown field of every wire type in every struct the decoder walks; returns
    [(case, plain blob, mutated struct's name)]: the records must equal the plain blob's."""
    out = []
    vals = unknown_values()
    k = 0
    for ev in family_events() + [None]:
        root = one_event_history(ev) if ev is not None else history(family_events())
        plain = blob(root)
        for path, st in structs(root):
            if ev is None and path != ():
                continue  # the many-event blob: only the History struct itself
            for vn, t, v in vals:
                where = ("before", "between", "after")[k % 3]
                fid = UNKNOWN_IDS[(k // 3) % len(UNKNOWN_IDS)]
                k += 1
                nm = "a/%s@%s/%s/%s/id%d" % (st.name, "-".join(map(str, path)) or "root", vn, where, fid)
                out.append(((nm, blob(insert_unknown(root, path, where, fid, t, v)), OK, STRICT), plain, st.name))
    return out


def wrong_type_cases():
    """(b) every field of every struct with another wire type on its id; returns
    [(case, the blob with that field removed)]: thriftrw ignores such a field."""
    out = []
    vals = unknown_values()
    k = 0

    def add(nm, root, path, pos, t, v, status=OK):
        def put(st):
            st.fields[pos] = F(t, st.fields[pos].fid, copy(v))

        def drop(st):
            del st.fields[pos]
        out.append(((nm, blob(edited(root, path, put)), status, STRICT), blob(edited(root, path, drop))))
    for ev in family_events():
        root = one_event_history(ev)
        for path, st in structs(root):
            if st.name == "Memo":
                continue  # kept as raw bytes: no field of it is read
            for pos, f in enumerate(st.fields):
                done = 0
                while done < 2:
                    vn, t, v = vals[k % len(vals)]
                    k += 1
                    if t == f.t:
                        continue
                    done += 1
                    status = TD.DEC_NO_EVENTS if st.name == "History" else OK
                    add("b/%s.%d-as-%s" % (st.name, f.fid, vn), root, path, pos, t, v, status)
    # the container fields with the right field type and other element types
    root = one_event_history(started(1))
    for path, st in structs(root):
        for pos, f in enumerate(st.fields):
            if st.name == "SearchAttributes":
                add("b/sa-map-i32-string", root, path, pos, T_MAP, Mp(T_I32, T_STRING, [(1, b"x"), (2, b"y")]))
                add("b/sa-map-string-i64", root, path, pos, T_MAP, Mp(T_STRING, T_I64, [(b"x", 1)]))
                add("b/sa-as-list", root, path, pos, T_LIST, Lst(T_STRING, [b"k1", b"v1"]))
            elif st.name == "ResetPoints":
                add("b/rps-list-i64", root, path, pos, T_LIST, Lst(T_I64, [1, 2, 3]))
            elif st.name == "RetryPolicy" and f.fid == 50:
                add("b/reasons-as-set", root, path, pos, T_SET, Lst(T_STRING, [b"bad", b"worse"]))
                add("b/reasons-empty-list", root, path, pos, T_LIST, Lst(T_STRING, []))
            elif st.name == "HistoryEvent" and f.fid == 10:
                add("b/eventId-as-i32", root, path, pos, T_I32, 1)
                add("b/eventId-as-string", root, path, pos, T_STRING, b"1")
            elif st.name == "attr40" and f.fid == 20:
                add("b/tasklist-as-string", root, path, pos, T_STRING, b"tl")
            elif st.name == "attr40" and f.fid == 40:
                add("b/attr-field-as-i64", root, path, pos, T_I64, 3600)
            elif st.name == "History":
                add("b/events-list-i64", root, path, pos, T_LIST, Lst(T_I64, [1, 2]), TD.DEC_NO_EVENTS)
                add("b/events-count-0", root, path, pos, T_LIST, Lst(T_STRUCT, []), TD.DEC_NO_EVENTS)
    return out


def _find(root, pred):
    return [(p, st) for p, st in structs(root) if pred(st)]


def repeated_cases():
    """(c) repeated fields; returns [(case, the blob with only the surviving occurrence)].
    The generated FromWire assigns each occurrence in turn and replaces a struct-valued
    field whole, so the expected records are those of the blob without the earlier one."""
    out = []

    def add(nm, root, path, pos, first: F):
        """`first` inserted before field `pos` of the struct at path; the survivor is the tree as is."""
        out.append(((nm, blob(edited(root, path, lambda st: st.fields.insert(pos, copy(first)))), OK, BY_STRING),
                    blob(root)))

    def pos_of(st, fid):
        return [i for i, f in enumerate(st.fields) if f.fid == fid][0]
    root = history([started(1), upsert(2)])
    (pe, ev), = _find(root, lambda st: st.name == "HistoryEvent" and st.fields[0].v == 1)
    (pa, a40), = _find(root, lambda st: st.name == "attr40")
    add("c/scalar-eventId", root, pe, 0, i64(10, 99))
    add("c/scalar-far-apart", root, pe, 0, i64(35, 99))
    add("c/scalar-initiator-flags", root, pa, pos_of(a40, 55), i32(55, 1))
    add("c/string-continuedRunId", root, pa, pos_of(a40, 54), s(54, b"older-run"))
    add("c/parent-domain", root, pa, pos_of(a40, 12), s(12, b"other-parent-domain"))
    add("c/tasklist", root, pa, pos_of(a40, 20), sub(20, "TaskList", [s(10, b"older-tl"), i32(20, 1)]))
    add("c/tasklist-first-has-name-only", root, pa, pos_of(a40, 10), name(10, "WorkflowType", b"older-wt"))
    add("c/parent-execution-second-lacks-runId", history([edited(
        started(1), (5,), lambda st: st.fields.__setitem__(2, sub(14, "WorkflowExecution", [s(10, b"pw")])))]),
        (0, 0, 5), 2, execution(14, b"older-pw", b"older-pr"))
    add("c/retry-policy-second-lacks-fields", history([edited(
        started(1), (5,), lambda st: st.fields.__setitem__(pos_of(st, 70), sub(70, "RetryPolicy", [i32(40, 9)])))]),
        (0, 0, 5), pos_of(a40, 70), retry_policy(70))
    add("c/memo", root, pa, pos_of(a40, 120), memo(120, [(b"older", b"memo")]))
    # a repeated attribute struct whose second occurrence lacks fields the first had
    small = history([event(1, 40, [name(20, "TaskList", b"tl"), i32(40, 7)]), upsert(2)])
    add("c/attr-struct-second-lacks-fields", small, (0, 0), 5, copy(started(1).fields[5]))
    add("c/attr-struct-second-longer", root, pe, 5, sub(40, "attr40", [name(20, "TaskList", b"tl0"), search_attributes(
        121, [(b"only", b"one")])]))
    # SearchAttributes twice in one attribute struct; the map twice in one SearchAttributes
    add("c/search-attributes-first-longer", root, pa, pos_of(a40, 121),
        search_attributes(121, [(b"o%d" % i, b"p%d" % i) for i in range(5)]))
    add("c/search-attributes-first-shorter", root, pa, pos_of(a40, 121), search_attributes(121, [(b"o", b"p")]))
    (psa, sa), = _find(root, lambda st: st.name == "SearchAttributes" and len(st.fields[0].v.pairs) == 2 and st.fields[
        0].v.pairs[0][0] == b"k1" and st.fields[0].v.pairs[0][1] == b"v1")
    add("c/sa-map-first-longer", root, psa, 0, mp(10, T_STRING, T_STRING, [(b"m%d" % i, b"n") for i in range(4)]))
    add("c/sa-map-first-shorter", root, psa, 0, mp(10, T_STRING, T_STRING, [(b"m", b"n")]))
    (pu, up), = _find(root, lambda st: st.name == "attr450")
    add("c/upsert-search-attributes", root, pu, 1, search_attributes(20, [(b"u%d" % i, b"w") for i in range(3)]))
    # ResetPoints twice; the list twice inside one ResetPoints; a later ResetPoints without points
    add("c/reset-points-first-longer", root, pa, pos_of(a40, 130),
        reset_points(130, [reset_point(b"oc%d" % k, b"or%d" % k, k) for k in range(4)]))
    add("c/reset-points-first-shorter", root, pa, pos_of(a40, 130), reset_points(130, [reset_point(b"oc", b"or", 1)]))
    (prp, rp), = _find(root, lambda st: st.name == "ResetPoints")
    add("c/reset-points-list-twice", root, prp, 0, lst(10, T_STRUCT, [reset_point(b"oc%d" % k, b"or", k) for k in range(3)]))
    norp = history([edited(started(1), (5,), lambda st: st.fields.__setitem__(pos_of(st, 130), sub(130, "ResetPoints", [])))])
    add("c/reset-points-second-empty", norp, (0, 0, 5), pos_of(a40, 130), reset_points(130, [reset_point(b"oc", b"or", 0)]))
    (pp, pt) = _find(root, lambda st: st.name == "ResetPointInfo")[1]  # its resettable is false
    add("c/reset-point-resettable", root, pp, 0, boolean(60, True))
    # two different attribute structs in one event: the record keeps the last
    add("c/two-attr-structs-upsert-then-started", root, pe, 5, copy(upsert(1).fields[5]))
    (pe2, ev2), = _find(root, lambda st: st.name == "HistoryEvent" and st.fields[0].v == 2)
    add("c/two-attr-structs-started-then-upsert", root, pe2, 5, copy(started(2, b"x").fields[5]))
    add("c/two-attr-structs-timer-then-upsert", root, pe2, 5, copy(timer_started(2).fields[5]))
    x = history([edited(cancel_initiated(1), (5,), lambda st: st.fields.__setitem__(3, boolean(50, False)))])
    add("c/external-childOnly", x, (0, 0, 5), 3, boolean(50, True))
    add("c/external-execution", x, (0, 0, 5), 1, execution(30, b"older-w", b"older-r"))
    return out


def repeated_list_cases():
    """(c, finding 2) History field 10 twice: the earlier list longer, shorter, equal, and
    an earlier list of structs before a list<i64> (no events).  Every event carries search
    attributes and reset points, so all three row ranges move."""
    def evs(n, tag):
        return [started(k + 1, tag + b"%d" % k, full=False) for k in range(n)]
    out = []
    for nm, n1, n2 in (("longer", 4, 1), ("shorter", 1, 3), ("equal", 2, 2), ("much-longer", 9, 2)):
        last = evs(n2, b"L")
        both = St("History", [lst(10, T_STRUCT, evs(n1, b"E")), lst(10, T_STRUCT, last)])
        out.append((("c/events-list-earlier-" + nm, blob(both), OK, BY_STRING), blob(history(last))))
    none = St("History", [lst(10, T_STRUCT, evs(3, b"E")), lst(10, T_I64, [1, 2])])
    out.append((("c/events-list-then-list-i64", blob(none), TD.DEC_NO_EVENTS, BY_STRING), blob(St("History", []))))
    ign = St("History", [lst(10, T_STRUCT, evs(2, b"L")), s(10, b"not a list")])
    out.append((("c/events-list-then-string", blob(ign), OK, BY_STRING), blob(history(evs(2, b"L")))))
    return out


# ------------------------------------------------------------------ depth
def nested(kind, levels):
    """(wire type, value) of `levels` containers nested in one another."""
    if kind == "struct":
        v = St("x", [])
        for _ in range(levels - 1):
            v = St("x", [F(T_STRUCT, 1, v)])
        return T_STRUCT, v
    if kind == "list":
        v = Lst(T_I32, [])
        for _ in range(levels - 1):
            v = Lst(T_LIST, [v])
        return T_LIST, v
    v = Mp(T_I32, T_I32, [])
    for _ in range(levels - 1):
        v = Mp(T_I32, T_MAP, [(1, v)])
    return T_MAP, v


DEPTH_PLACES = ("History", "HistoryEvent", "attr40", "RetryPolicy", "Memo")


def depth_cases():
    """(d) 11..18 nested structs / lists / map values in an unknown field at each place a
    skip starts, and inside Memo (kept as raw bytes through the same skipper: the Memo
    struct is level 1 there).  [(case, place, kind, levels)]; a value of more than
    CDR_THRIFT_MAX_DEPTH levels fails with DEPTH (cdr/ingest.h, Depth)."""
    root = one_event_history(started(1))
    out = []
    for place in DEPTH_PLACES:
        (path, st) = _find(root, lambda x: x.name == place)[0]
        for kind in ("struct", "list", "map"):
            for levels in range(11, 19):
                t, v = nested(kind, levels - 1 if place == "Memo" else levels)
                b = blob(insert_unknown(root, path, ("before", "between", "after")[levels % 3], 77, t, v))
                status = OK if levels <= TD.MAX_DEPTH else TD.DEC_DEPTH
                out.append((("d/%s/%s/%d" % (place, kind, levels), b, status, STRICT), place, kind, levels))
    return out


# ------------------------------------------------------------------ prefixes and bytes
def small_history():
    """(e) a started event with retry policy, memo, two search attributes and two reset
    points, one event of each other family, one unknown struct field: eleven events with
    one-byte strings and only the event id and type in front of each attribute struct,
    which is as small as that content gets (about 600 bytes)."""
    st = event(1, 40, [name(10, "WorkflowType", b"w"), name(20, "TaskList", b"t"), sub(70, "RetryPolicy", [
        i32(10, 2), lst(50, T_STRING, [b"e"])]), memo(120, [(b"m", b"n")]), search_attributes(121, [(b"a", b"b"), (b"c", b"d")]),
        reset_points(130, [St("ResetPointInfo", [s(10, b"x"), boolean(60, True)]), St("ResetPointInfo", [s(20, b"y")])])])
    small = lambda eid, attr, f: St("HistoryEvent", [i64(10, eid), i32(30, abi.EV[ATTR_TYPE[attr]]),  # noqa: E731
                                                     sub(attr, "attr%d" % attr, f)])
    st.fields = [st.fields[0], st.fields[2], st.fields[5]]
    evs = [st, small(3, 100, [i64(20, 2), s(50, b"k")]),
           small(4, 130, [s(10, b"a"), name(30, "TaskList", b"t")]), small(5, 150, [i64(20, 4)]),
           small(6, 180, [s(10, b"r"), i64(20, 9)]), small(7, 340, [s(10, b"d"), s(20, b"c")]),
           small(8, 420, [s(20, b"d"), execution(30, b"w", b"r")]), small(9, 300, [s(20, b"d"), boolean(50, True)]),
           small(10, 370, [execution(30, b"w", b"r"), i64(50, 7)]), small(11, 330, [s(10, b"n")]),
           small(12, 450, [search_attributes(20, [(b"a", b"z")])])]
    evs[3].fields.append(sub(99, "x", [i32(1, 1), lst(2, T_STRING, [b"q"])]))
    return history(evs)


MUTATION_BYTES = (0x00, 0x0B, 0x0C, 0x0D, 0x0F, 0x7F, 0x80, 0xFF)


def event_boundaries(root: St):
    """Byte offsets in blob(root) just after each event of History field 10 (the list first)."""
    assert root.fields[0].fid == 10
    p = 1 + 3 + 5
    out = []
    for ev in root.fields[0].v.items:
        p += len(value(T_STRUCT, ev))
        out.append(p)
    return out


def restored(b: bytes, cut: int, k: int) -> bytes:
    """The prefix b[:cut] ending after event k of the list at offset 4, with the closing
    bytes restored: the list's count set to k and the History stop byte appended."""
    return b[:5] + struct.pack(">i", k) + b[9:cut] + b"\x00"
