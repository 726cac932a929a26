"""The target lines of one prediction slice as two integer arrays -- built from the remapped log on the device
(csrc/targetgen.hip) or on the host (dataprep.gen_target_lines(draws="cell")), the same words either way -- which the loaders
take as they are: DeviceGraphLoader and PointLogStore accept a TargetStore where they accept target lines, without a Python
list in between.  Replaces gen_target.py:79-121 (target_<t>.txt), :277-290 (the pop list) and sampling.py:31-37 (the _sample
files) for the training loop.  UserNegLists is CCMR's user_neg_dict (feateng_ccmr.py:173-183), the negatives a line takes
before any draw (gen_target.py:79-96).
"""
import ctypes as C

import numpy as np

from . import dataprep
from .placement import check_build, device_as, device_i32, device_of
from .placement import is_tensor as _is_tensor, to_host as _host


def pop_items_device(graph, pop_standard, max_iid=None):
    """dataprep.gen_pop_items on a graph built on the device (TemporalGraph.from_log(build="device")): score_pop_items over
    its resident item-side off1 -> device int32 tensor [n_pop]; the list never leaves the device."""
    import torch
    from . import _lib
    b, dev = graph._built, graph._built_device
    lib = _lib.load()
    with torch.cuda.device(dev):
        temp, temp_bytes = _lib.workspace("score_pop_items", dev, graph.I)
        a = _lib.PopItems(C.sizeof(_lib.PopItems), b["i_off1"].data_ptr(), graph.U, graph.I, graph.S, int(pop_standard),
                          int(max_iid) if max_iid is not None else 2 ** 31 - 1, 0)
        stream = _lib.current_stream(dev)
        n_pop = C.c_int64(-1)
        _lib.check(lib.score_pop_items(C.byref(a), None, 0, C.byref(n_pop), temp.data_ptr(), temp_bytes, stream),
                   "score_pop_items (count)")
        pop = torch.empty((int(n_pop.value),), dtype=torch.int32, device=dev)
        if n_pop.value:
            _lib.check(lib.score_pop_items(C.byref(a), pop.data_ptr(), int(n_pop.value), None, temp.data_ptr(), temp_bytes, stream),
                       "score_pop_items (fill)")
            torch.cuda.current_stream(dev).synchronize()          # (temp is released behind this)
    return pop


class UserNegLists(object):
    """user_neg_dict (feateng_ccmr.py:173-183) as a CSR over uid = 1 .. n_users: off int64 [n_users + 1], items int32; the
    negatively rated items of uid u are items[off[u - 1]:off[u]], in log order, duplicates kept, not cut by time (the reference
    reads the whole negative file).  off[n_users] entries of items are used.  numpy arrays, or tensors on the device.

    gen_target_lines(draws="stream", neg_lists=...) APPENDS its random pads to the lists, as gen_user_neg_items appends them to
    the list inside the reference's dict (gen_target.py:89-95): the object is mutated, and a later split sees the pads."""

    def __init__(self, off, items, n_users):
        self.off, self.items, self.n_users = off, items, int(n_users)
        if int(off.shape[0]) != self.n_users + 1:
            raise ValueError("off must hold n_users + 1 = %d entries, got %d" % (self.n_users + 1, int(off.shape[0])))

    on_device = property(lambda self: _is_tensor(self.off))

    @classmethod
    def empty(cls, n_users):
        return cls(np.zeros(int(n_users) + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), n_users)

    @classmethod
    def from_events(cls, neg_uid, neg_iid, n_users, build="host", device=None):
        """neg_uid / neg_iid: the negative events in log order (remap_ccmr_log's).  An event whose uid lies outside
        1 .. n_users joins no list.  build="device" (needs a GPU): score_neg_lists_build on int32 tensors (uploaded if they are
        not there yet); off and items stay on the device."""
        check_build(build)
        U = int(n_users)
        if U <= 0:
            raise ValueError("n_users must be positive")
        if build == "host":
            u, i = _host(neg_uid).astype(np.int64).ravel(), _host(neg_iid).astype(np.int64).ravel()
            if len(u) != len(i):
                raise ValueError("neg_uid and neg_iid must be of one length")
            ok = (u >= 1) & (u <= U)
            u, i = u[ok], i[ok]
            order = np.argsort(u, kind="stable")
            off = np.zeros(U + 1, dtype=np.int64)
            np.cumsum(np.bincount(u - 1, minlength=U), out=off[1:])
            return cls(off, i[order].astype(np.int32), U)
        import torch
        from . import _lib
        dev = device_of(device, "UserNegLists.from_events(build='device')", like=neg_uid)
        lib = _lib.load()
        with torch.cuda.device(dev):
            d_u, d_i = device_i32(neg_uid, dev), device_i32(neg_iid, dev)
            n = int(d_u.numel())
            if int(d_i.numel()) != n:
                raise ValueError("neg_uid and neg_iid must be of one length")
            temp, temp_bytes = _lib.workspace("score_neg_lists", dev, n)
            off = torch.empty((U + 1,), dtype=torch.int64, device=dev)
            items = torch.empty((n,), dtype=torch.int32, device=dev)
            ptr = lambda t: t.data_ptr() if n else None
            _lib.check(lib.score_neg_lists_build(ptr(d_u), ptr(d_i), n, U, off.data_ptr(), ptr(items), temp.data_ptr(), temp_bytes,
                                                 _lib.current_stream(dev)), "score_neg_lists_build")
            torch.cuda.current_stream(dev).synchronize()          # (temp and uploaded columns are released behind this)
        return cls(off, items, U)

    def arrays(self):
        """(off int64, items int32) as numpy"""
        return _host(self.off).astype(np.int64), _host(self.items).astype(np.int32)

    def device_tensors(self, device):
        """(off int64, items int32) as tensors on `device`: the object's own where it lives there"""
        return device_as(self.off, device, np.int64), device_as(self.items, device, np.int32)

    def lists(self):
        """{uid: [iid, ...]} of the users with at least one entry: the dict form"""
        off, items = self.arrays()
        return {u + 1: items[off[u]:off[u + 1]].tolist() for u in np.flatnonzero(np.diff(off) > 0).tolist()}

    def _append(self, pads):
        """pads {uid: [iid, ...]} go behind the users' lists (the stream rule; host lists only)"""
        if not pads:
            return
        lists = self.lists()
        for u, extra in pads.items():
            lists[u] = lists.get(u, []) + [int(x) for x in extra]
        lens = np.zeros(self.n_users, dtype=np.int64)
        for u, l in lists.items():
            lens[u - 1] = len(l)
        new_off = np.zeros(self.n_users + 1, dtype=np.int64)
        np.cumsum(lens, out=new_off[1:])
        self.off = new_off
        self.items = np.asarray([x for u in sorted(lists) for x in lists[u]], dtype=np.int32)


class TargetStore(object):
    """line_user int32 [n_lines] and line_items int32 [n_lines, per_line] (the positive, then per_line - 1 negatives), numpy
    arrays or device tensors; n_lines, per_line."""

    def __init__(self, line_user, line_items, per_line=None):
        self.line_user, self.line_items = line_user, line_items
        self.n_lines = int(line_user.shape[0])
        self.per_line = int(per_line if per_line is not None else line_items.shape[1])
        if tuple(line_items.shape) != (self.n_lines, self.per_line):
            raise ValueError("line_items must be [n_lines, per_line] = %r, got %r"
                             % ((self.n_lines, self.per_line), tuple(line_items.shape)))
        self._lines = None

    neg_sample_num = property(lambda self: self.per_line - 1)
    on_device = property(lambda self: _is_tensor(self.line_user))

    @classmethod
    def from_log(cls, uid, iid, t_idx, n_users, n_items, pred_time, neg_sample_num, start_time=0, seed=11, build="device",
                 pop_items=None, sample_factor=None, device=None, neg_lists=None):
        """The lines dataprep.gen_target_lines(draws="cell") yields, after dataprep.sample_target_lines(draws="cell") where
        sample_factor is given (same seed).  build="host": numpy, those two functions; build="device" (needs a GPU):
        score_target_build, the same words.  uid / iid / t_idx: numpy arrays or int32 tensors already on the device -- one
        upload serves the graph and the targets.  pop_items: None, an array, a device tensor or (graph, pop_standard) --
        dataprep.gen_pop_items, evaluated on the device where the graph was built there.  ValueError: a sample_factor below
        1; an empty pop list with at least one line to fill.  On both builds that means a line LEFT by the down-sampling (the
        device learns the count of those alone); gen_target_lines itself, which knows nothing of a sample_factor, raises as
        soon as any user is eligible.  neg_lists: a UserNegLists (CCMR): gen_target_lines' -- a line's first negatives are the
        user's own, the draws fill the rest; on the device score_target_build_lists, the lists uploaded where they are not
        there yet."""
        check_build(build)
        if sample_factor is not None and int(sample_factor) < 1:
            raise ValueError("sample_factor must be at least 1: got %r" % (sample_factor,))
        U, I, neg = int(n_users), int(n_items), int(neg_sample_num)
        if neg < 0:
            raise ValueError("neg_sample_num must not be negative")
        if build == "host":
            pop = pop_items
            if isinstance(pop, tuple):
                pop = dataprep.gen_pop_items(pop[0], pop[1])
            elif pop is not None:
                pop = _host(pop)
            empty_pop = pop is not None and len(pop) == 0        # (an error only if a line is left after the down-sampling)
            lines = dataprep.gen_target_lines(_host(uid), _host(iid), _host(t_idx), U, I, pred_time, neg, start_time, seed,
                                              draws="cell", pop_items=None if empty_pop else pop, neg_lists=neg_lists)
            if sample_factor is not None:
                lines = dataprep.sample_target_lines(lines, sample_factor, seed, draws="cell")
            if empty_pop and lines:
                raise ValueError("pop_items is empty and %d users are eligible" % len(lines))
            return cls._from_lines(lines, 1 + neg)
        import torch
        from . import _lib
        dev = device_of(device, "TargetStore.from_log(build='device')", like=uid)
        lib = _lib.load()

        up = lambda a: device_i32(a, dev)
        with torch.cuda.device(dev):
            d_uid, d_iid, d_t = up(uid), up(iid), up(t_idx)
            n = int(d_uid.numel())
            if n == 0 or d_iid.numel() != n or d_t.numel() != n:
                raise ValueError("from_log(build='device'): uid, iid and t_idx must be non-empty and of one length")
            if isinstance(pop_items, tuple):
                g, standard = pop_items
                if g._built is not None and g._built_device == dev:
                    d_pop = pop_items_device(g, standard)
                else:
                    d_pop = up(dataprep.gen_pop_items(g, standard))
            else:
                d_pop = None if pop_items is None else up(pop_items)
            n_pop = 0 if d_pop is None else int(d_pop.numel())
            pop_arg = None if d_pop is None else d_pop if n_pop else torch.zeros((1,), dtype=torch.int32, device=dev)
            temp, temp_bytes = _lib.workspace("score_target_build", dev, n, U)
            a = _lib.TargetBuild(C.sizeof(_lib.TargetBuild), d_uid.data_ptr(), d_iid.data_ptr(), d_t.data_ptr(), n, U, I,
                                 int(start_time), int(pred_time), neg, int(sample_factor or 0), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                 None if pop_arg is None else pop_arg.data_ptr(), n_pop)
            stream = _lib.current_stream(dev)
            n_lines = C.c_int64(-1)
            call, what = lib.score_target_build, "score_target_build"
            if neg_lists is not None:
                if neg_lists.n_users != U:
                    raise ValueError("neg_lists is over %d users, the log over %d" % (neg_lists.n_users, U))
                d_off, d_items = neg_lists.device_tensors(dev)
                d_off, d_items = d_off.contiguous(), d_items.contiguous()
                n_neg = int(d_items.numel())
                a = _lib.TargetLists(C.sizeof(_lib.TargetLists), a, d_off.data_ptr(), d_items.data_ptr() if n_neg else None, n_neg)
                call, what = lib.score_target_build_lists, "score_target_build_lists"
            _lib.check(call(C.byref(a), None, None, 0, C.byref(n_lines), temp.data_ptr(), temp_bytes, stream), what + " (count)")
            L = int(n_lines.value)
            if L and d_pop is not None and n_pop == 0:
                raise ValueError("pop_items is empty and %d users are eligible" % L)
            line_user = torch.empty((L,), dtype=torch.int32, device=dev)
            line_items = torch.empty((L, 1 + neg), dtype=torch.int32, device=dev)
            if L:
                _lib.check(call(C.byref(a), line_user.data_ptr(), line_items.data_ptr(), L, None, temp.data_ptr(), temp_bytes,
                                stream), what + " (fill)")
                torch.cuda.current_stream(dev).synchronize()      # (temp and an uploaded log are released behind this)
        return cls(line_user, line_items, 1 + neg)

    @classmethod
    def _from_lines(cls, lines, per_line=None):
        if per_line is None:
            if not lines:
                raise ValueError("no lines: per_line is unknown")
            per_line = len(lines[0][1])
        lu = np.asarray([int(u) for u, _ in lines], dtype=np.int32)
        li = np.asarray([its for _, its in lines], dtype=np.int32).reshape(len(lines), per_line)
        return cls(lu, li, per_line)

    def arrays(self):
        """(line_user, line_items) as numpy"""
        return _host(self.line_user), _host(self.line_items)

    def device_tensors(self, device):
        """(line_user, line_items) as int32 tensors on `device`: the store's own where it lives there"""
        return device_as(self.line_user, device, np.int32), device_as(self.line_items, device, np.int32)

    def lines(self):
        """[(uid, [pos, neg...])], what dataprep.gen_target_lines yields; a device store downloads on first use"""
        if self._lines is None:
            lu, li = self.arrays()
            self._lines = list(zip(lu.tolist(), li.tolist()))
        return self._lines

    def save(self, path):
        """target_<t>.txt's format (gen_target.py:118): 'uid,pos,neg...' and a newline per line"""
        with open(path, "w") as f:
            f.write("".join("%d,%s\n" % (u, ",".join(map(str, its))) for u, its in self.lines()))
        return path

    @classmethod
    def load(cls, path):
        with open(path, "r") as f:
            rows = [[int(x) for x in l.strip().split(",")] for l in f if l.strip()]
        if not rows or any(len(r) != len(rows[0]) or len(r) < 2 for r in rows):
            raise ValueError("%s: every line must be 'uid,pos,neg...' with one number of items" % path)
        return cls._from_lines([(r[0], r[1:]) for r in rows])
