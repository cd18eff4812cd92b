"""The sequence of entry-point calls a callable makes, in a form that compares across runs and commits."""
import ctypes

from yolo_dual_amd import _lib as L


def launch_trace(fn):
    """Run ``fn()`` with a recorder installed through ``_lib.set_recorder`` and return its operations in order, each a list:
    * a call: the entry-point name, then one value per argument by its type in ``_lib.SIGNATURES`` — an integer is itself, a float its
      ``float.hex``, a ConvGeom its 13 fields, a BnRed ``nseg`` and its integer arrays, any other pointer 0 (null) or 1, and the stream
      (the last argument) its slot number in order of first appearance;
    * a cross-stream edge (``tape.stream_wait``): "edge", the slot waited on, the waiting slot.
    Buffer addresses are left out on purpose: the order of scratch allocations is not part of what the GPU executes."""
    ops, slots = [], {}

    def raw(a):
        return int(getattr(a, "value", a) or 0)

    def slot(handle):
        return slots.setdefault(raw(handle), len(slots))

    def struct(a):
        obj = getattr(a, "_obj", None)
        return a.contents if obj is None else obj

    class Rec:
        @staticmethod
        def add(name, args):
            argtypes = L.SIGNATURES[name][1]
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            op = [name]
            for a, t in zip(args[:-1], argtypes[:-1]):
                if t is L._G:
                    g = struct(a)
                    op += [getattr(g, f) for f, _ in L.ConvGeom._fields_]
                elif t is L._R:
                    r = struct(a)
                    op += [r.nseg] + [list(getattr(r, f)) for f in ("c0", "c1", "ldy", "cp", "act")]
                elif t is L._f or t is L._d:
                    op.append(float(getattr(a, "value", a)).hex())
                elif t is L._vp or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
                    op.append(int(raw(a) != 0))
                else:
                    op.append(raw(a))
            op.append(slot(args[-1]))
            ops.append(op)

        @staticmethod
        def edge(src, dst):
            ops.append(["edge", slot(src), slot(dst)])

    before = L.recorder()
    L.set_recorder(Rec)
    try:
        fn()
    finally:
        L.set_recorder(before)
    return ops
