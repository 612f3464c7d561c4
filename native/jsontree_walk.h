// The copy and merge walks over wire-format JSON trees (dict/list/scalars),
// shared by jsontree.cpp (which exports them) and revstore.cpp (which runs
// them inside the apiserver's write verbs). Raw CPython C API, header only.
#ifndef GPU_PROVISIONER_AMD_JSONTREE_WALK_H
#define GPU_PROVISIONER_AMD_JSONTREE_WALK_H

#define PY_SSIZE_T_CLEAN
#include <Python.h>

// Internal linkage on purpose: each extension keeps its own copy, so the
// recursive calls bind directly instead of through the shared object's
// symbol table (these walks recurse once per container).
namespace jsontree_walk {

// ---------------------------------------------------------------------------
// deep_copy
// ---------------------------------------------------------------------------

static inline bool is_container(PyObject* o) {
    return PyDict_CheckExact(o) || PyList_CheckExact(o);
}

// Exact dict/list are copied recursively; everything else (subclasses,
// tuples, scalars) is returned as the same object. Each level first takes a
// private shallow copy and then replaces container values in it, so the
// input is never iterated while other code could run.
static inline PyObject* copy_tree(PyObject* o) {
    if (PyDict_CheckExact(o)) {
        if (Py_EnterRecursiveCall(" while copying a JSON tree")) return nullptr;
        PyObject* out = PyDict_Copy(o);
        if (out != nullptr) {
            Py_ssize_t pos = 0;
            PyObject *k, *v;
            // replacing the value of an existing key is allowed during PyDict_Next
            while (PyDict_Next(out, &pos, &k, &v)) {
                if (!is_container(v)) continue;
                PyObject* nv = copy_tree(v);
                if (nv == nullptr || PyDict_SetItem(out, k, nv) < 0) {
                    Py_XDECREF(nv);
                    Py_CLEAR(out);
                    break;
                }
                Py_DECREF(nv);
            }
        }
        Py_LeaveRecursiveCall();
        return out;
    }
    if (PyList_CheckExact(o)) {
        if (Py_EnterRecursiveCall(" while copying a JSON tree")) return nullptr;
        PyObject* out = PyList_GetSlice(o, 0, PyList_GET_SIZE(o));
        if (out != nullptr) {
            Py_ssize_t n = PyList_GET_SIZE(out);
            for (Py_ssize_t i = 0; i < n; i++) {
                PyObject* v = PyList_GET_ITEM(out, i);
                if (!is_container(v)) continue;
                PyObject* nv = copy_tree(v);
                if (nv == nullptr) {
                    Py_CLEAR(out);
                    break;
                }
                PyList_SET_ITEM(out, i, nv);
                Py_DECREF(v);
            }
        }
        Py_LeaveRecursiveCall();
        return out;
    }
    Py_INCREF(o);
    return o;
}

// ---------------------------------------------------------------------------
// merge patch (RFC 7386)
// ---------------------------------------------------------------------------

// dict(target) when target is a dict (any subclass), else {}. target may be
// nullptr ("key absent": the Python code merges into a fresh {}).
static inline PyObject* dict_of(PyObject* target) {
    if (target == nullptr || !PyDict_Check(target)) return PyDict_New();
    if (PyDict_CheckExact(target)) return PyDict_Copy(target);
    return PyObject_CallOneArg((PyObject*)&PyDict_Type, target);
}

static inline PyObject* merge(PyObject* target, PyObject* patch, bool owned);

// one (k, v) of the patch applied to `out`
static inline int merge_item(PyObject* out, PyObject* k, PyObject* v, bool owned) {
    if (v == Py_None) {
        if (PyDict_DelItem(out, k) < 0) {
            if (!PyErr_ExceptionMatches(PyExc_KeyError)) return -1;
            PyErr_Clear();
        }
        return 0;
    }
    PyObject* nv;
    if (PyDict_Check(v)) {
        PyObject* sub = PyDict_GetItemWithError(out, k);  // borrowed
        if (sub == nullptr && PyErr_Occurred()) return -1;
        Py_XINCREF(sub);
        nv = merge(sub, v, owned);
        Py_XDECREF(sub);
    } else if (owned) {
        nv = copy_tree(v);
    } else {
        Py_INCREF(v);
        nv = v;
    }
    if (nv == nullptr) return -1;
    int rc = PyDict_SetItem(out, k, nv);
    Py_DECREF(nv);
    return rc;
}

// json_merge_patch(target, patch); with owned=true every value taken from
// the patch is deep-copied on the way in, so the result holds no mutable
// object of the caller's patch while untouched target subtrees stay shared.
static inline PyObject* merge(PyObject* target, PyObject* patch, bool owned) {
    if (!PyDict_Check(patch)) {
        if (owned) return copy_tree(patch);
        Py_INCREF(patch);
        return patch;
    }
    if (Py_EnterRecursiveCall(" while applying a merge patch")) return nullptr;
    PyObject* out = dict_of(target);
    if (out != nullptr) {
        bool ok = true;
        if (PyDict_CheckExact(patch)) {
            Py_ssize_t pos = 0;
            PyObject *k, *v;
            while (ok && PyDict_Next(patch, &pos, &k, &v)) {
                Py_INCREF(k);
                Py_INCREF(v);
                ok = merge_item(out, k, v, owned) == 0;
                Py_DECREF(k);
                Py_DECREF(v);
            }
        } else {
            // dict subclass: go through its own items(), as the Python code does
            PyObject* items = PyObject_CallMethod(patch, "items", nullptr);
            PyObject* it = items ? PyObject_GetIter(items) : nullptr;
            Py_XDECREF(items);
            ok = it != nullptr;
            PyObject* kv;
            while (ok && (kv = PyIter_Next(it)) != nullptr) {
                PyObject* seq = PySequence_Fast(kv, "items() must yield pairs");
                Py_DECREF(kv);
                if (seq == nullptr || PySequence_Fast_GET_SIZE(seq) != 2) {
                    if (seq != nullptr) PyErr_SetString(PyExc_ValueError, "items() must yield pairs");
                    Py_XDECREF(seq);
                    ok = false;
                    break;
                }
                ok = merge_item(out, PySequence_Fast_GET_ITEM(seq, 0),
                                PySequence_Fast_GET_ITEM(seq, 1), owned) == 0;
                Py_DECREF(seq);
            }
            if (ok && PyErr_Occurred()) ok = false;
            Py_XDECREF(it);
        }
        if (!ok) Py_CLEAR(out);
    }
    Py_LeaveRecursiveCall();
    return out;
}

// merge_patch_owned(cur, patch): the owned merge of a whole object.
// `str_metadata` is the caller's interned "metadata".
static inline PyObject* merge_owned(PyObject* cur, PyObject* patch, PyObject* str_metadata) {
    PyObject* out = merge(cur, patch, true);
    if (out == nullptr || !PyDict_CheckExact(out) || !PyDict_Check(cur)) return out;
    // the caller writes into the top level and into metadata: metadata must
    // not be the stored revision's dict even when the patch left it alone
    PyObject* m = PyDict_GetItemWithError(out, str_metadata);
    if (m == nullptr) {
        if (PyErr_Occurred()) Py_CLEAR(out);
        return out;
    }
    if (PyDict_CheckExact(m) && m == PyDict_GetItemWithError(cur, str_metadata)) {
        PyObject* fresh = PyDict_Copy(m);
        if (fresh == nullptr || PyDict_SetItem(out, str_metadata, fresh) < 0) Py_CLEAR(out);
        Py_XDECREF(fresh);
    } else if (PyErr_Occurred()) {
        Py_CLEAR(out);
    }
    return out;
}

}  // namespace jsontree_walk

#endif  // GPU_PROVISIONER_AMD_JSONTREE_WALK_H
