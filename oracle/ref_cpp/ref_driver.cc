// TEST INFRASTRUCTURE ONLY -- drives the reference's C++ row writer and reader
// (cpp/fury/row/{row,writer,type}.cc, compiled in place from the reference tree by the Makefile
// beside this file) over the batches of Arrow-style columns the rest of this project speaks
// (fury_field / fury_column of include/fury_row.h), so the C restatement in oracle/row_oracle.c and
// the device path can be compared with an implementation of the row format that this project did
// not write.  FMT = java/fury-format/src/main/java/org/apache/fury/format.
//
//   ref_encode         each row through RowWriter / ArrayWriter: a nested struct through a child
//                      RowWriter, a list through an ArrayWriter, a map as WriteDirectly(-1), the key
//                      array, the key array's size patched into that word, the value array
//                      (Writer::WriteDirectly, writer.cc:95-103; the Java writer does the same,
//                      FMT/encoder/BaseBinaryEncoderBuilder.java:298-357).
//   ref_decode         each row through Row::PointTo and the Getter methods only (row.h:39-105).
//   ref_row_to_string  Row::ToString of one row (row.cc:146-168).
//
// Null fields.  Writer::SetNullAt only sets the bit (writer.h:64-66), and so does the Java
// BinaryWriter.setNullAt (FMT/row/binary/writer/BinaryWriter.java:123-129: "no need to put zero
// into the corresponding field").  The Java row's null slot is nevertheless 0, because
// RowEncoder.toRow hands the writer a fresh, zero-filled buffer for every row
// (FMT/encoder/Encoders.java:88-93, MemoryUtils.buffer) -- the canonical bytes of this project.
// The C++ Buffer is malloc'ed and RowWriter::Reset clears only the bitmap (writer.cc:124-132), so
// the driver writes the zero slot itself before SetNullAt.  ArrayWriter::Reset zeroes every element
// (writer.cc:224-227): a null element is SetNullAt alone.
//
// Two places where the C++ sibling's element width differs from the Java writer's
// (get_byte_width, cpp/fury/row/type.cc:37-43, against DataTypes.getTypeWidth,
// FMT/type/DataTypes.java:68-133; the table in DESIGN.md section 5):
//   decimal128  C++ 16 (a FixedWidthType), Java -1 (variable section): DECIMAL is refused here.
//   bool        C++ bit_width() / CHAR_BIT = 0, Java 1 (:88-90).  An ArrayWriter / ArrayData over
//               list<bool> therefore has 0-byte elements.  Lists and map sides of BOOL are declared
//               to the reference as list<int8> -- the Java width -- and written with
//               ArrayWriter::Write(int, bool) / read with Getter::GetBoolean, so the header, the
//               null bits and the padding of such arrays still come from the reference; the
//               one-byte stride itself is the Java reading, not the C++ one.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fury/row/row.h"
#include "fury/row/type.h"
#include "fury/row/writer.h"
#include "fury/util/buffer.h"
#include "fury_row.h"

namespace {

constexpr int64_t kErrUnsupported = -FURY_ERR_UNSUPPORTED;
constexpr int64_t kErrCapacity = -FURY_ERR_CAPACITY;

using TypePtr = std::shared_ptr<arrow::DataType>;

bool supported(const fury_field &f) {
  switch (f.type_id) {
  case FURY_TYPE_BOOL: case FURY_TYPE_INT8: case FURY_TYPE_INT16: case FURY_TYPE_INT32:
  case FURY_TYPE_INT64: case FURY_TYPE_FLOAT32: case FURY_TYPE_FLOAT64: case FURY_TYPE_STRING:
  case FURY_TYPE_BINARY: case FURY_TYPE_DATE32: case FURY_TYPE_TIMESTAMP:
    return f.num_children == 0;
  case FURY_TYPE_LIST:
    return f.num_children == 1 && supported(f.children[0]);
  case FURY_TYPE_MAP:
    return f.num_children == 2 && supported(f.children[0]) && supported(f.children[1]);
  case FURY_TYPE_STRUCT:
    for (int k = 0; k < f.num_children; k++) {
      if (!supported(f.children[k])) return false;
    }
    return true;
  default:
    return false; // DECIMAL and anything unknown
  }
}

TypePtr arrow_type(const fury_field &f);

// The type of an array's elements as declared to ArrayWriter / ArrayData: BOOL as int8 (header).
TypePtr element_type(const fury_field &f) {
  return f.type_id == FURY_TYPE_BOOL ? arrow::int8() : arrow_type(f);
}

std::shared_ptr<arrow::Field> arrow_field(const fury_field &f) {
  return arrow::field(f.name ? f.name : "", arrow_type(f), f.nullable != 0);
}

std::vector<std::shared_ptr<arrow::Field>> arrow_fields(const fury_field *fields, int n) {
  std::vector<std::shared_ptr<arrow::Field>> out;
  for (int k = 0; k < n; k++) out.push_back(arrow_field(fields[k]));
  return out;
}

TypePtr arrow_type(const fury_field &f) {
  switch (f.type_id) {
  case FURY_TYPE_BOOL: return arrow::boolean();
  case FURY_TYPE_INT8: return arrow::int8();
  case FURY_TYPE_INT16: return arrow::int16();
  case FURY_TYPE_INT32: return arrow::int32();
  case FURY_TYPE_INT64: return arrow::int64();
  case FURY_TYPE_FLOAT32: return arrow::float32();
  case FURY_TYPE_FLOAT64: return arrow::float64();
  case FURY_TYPE_STRING: return arrow::utf8();
  case FURY_TYPE_BINARY: return arrow::binary();
  case FURY_TYPE_DATE32: return arrow::date32();
  case FURY_TYPE_TIMESTAMP: return arrow::timestamp(arrow::TimeUnit::MICRO);
  case FURY_TYPE_LIST: return fury::list(element_type(f.children[0]));
  case FURY_TYPE_MAP: return fury::map(element_type(f.children[0]), element_type(f.children[1]));
  default: return arrow::struct_(arrow_fields(f.children, f.num_children));
  }
}

bool col_valid(const fury_column *c, int64_t i) {
  return c->validity == nullptr || ((c->validity[i >> 3] >> (i & 7)) & 1);
}

template <typename T> T load(const void *base, int64_t i) {
  T v;
  std::memcpy(&v, static_cast<const uint8_t *>(base) + i * static_cast<int64_t>(sizeof(T)),
              sizeof(T));
  return v;
}

// ---- encode ------------------------------------------------------------------------------
// One writer per schema node, built once and reused for every row, the way the reference nests
// them: a child writer shares its parent's buffer and is registered with it, so SetBuffer on the
// top RowWriter reaches all of them (writer.h:117-122).
struct Node {
  const fury_field *f = nullptr;
  std::unique_ptr<fury::RowWriter> row;    // STRUCT
  std::unique_ptr<fury::ArrayWriter> arr;  // LIST elements; MAP keys
  std::unique_ptr<fury::ArrayWriter> varr; // MAP values
  std::vector<Node> kids;
};

void build_node(Node &nd, const fury_field &f, fury::Writer *parent) {
  nd.f = &f;
  nd.kids.resize(static_cast<size_t>(f.num_children));
  if (f.type_id == FURY_TYPE_STRUCT) {
    nd.row = std::make_unique<fury::RowWriter>(
        arrow::schema(arrow_fields(f.children, f.num_children)), parent);
    for (int k = 0; k < f.num_children; k++) build_node(nd.kids[k], f.children[k], nd.row.get());
  } else if (f.type_id == FURY_TYPE_LIST) {
    nd.arr = std::make_unique<fury::ArrayWriter>(fury::list(element_type(f.children[0])), parent);
    build_node(nd.kids[0], f.children[0], nd.arr.get());
  } else if (f.type_id == FURY_TYPE_MAP) {
    nd.arr = std::make_unique<fury::ArrayWriter>(fury::list(element_type(f.children[0])), parent);
    nd.varr = std::make_unique<fury::ArrayWriter>(fury::list(element_type(f.children[1])), parent);
    build_node(nd.kids[0], f.children[0], nd.arr.get());
    build_node(nd.kids[1], f.children[1], nd.varr.get());
  }
}

void write_value(fury::Writer *w, bool in_array, int ord, Node &nd, const fury_column *c, int64_t i);

void write_array(fury::ArrayWriter *aw, Node &elem, const fury_column *child, int64_t begin,
                 int64_t end) {
  aw->Reset(static_cast<uint32_t>(end - begin));
  for (int64_t j = begin; j < end; j++) {
    write_value(aw, true, static_cast<int>(j - begin), elem, child, j);
  }
}

void write_value(fury::Writer *w, bool in_array, int ord, Node &nd, const fury_column *c,
                 int64_t i) {
  const fury_field &f = *nd.f;
  if (!col_valid(c, i)) {
    if (!in_array) w->Write(ord, static_cast<int64_t>(0)); // the zero slot (header)
    w->SetNullAt(ord);
    return;
  }
  switch (f.type_id) {
  case FURY_TYPE_BOOL: {
    const uint8_t *bits = static_cast<const uint8_t *>(c->values);
    w->Write(ord, static_cast<bool>((bits[i >> 3] >> (i & 7)) & 1));
    return;
  }
  case FURY_TYPE_INT8: w->Write(ord, load<int8_t>(c->values, i)); return;
  case FURY_TYPE_INT16: w->Write(ord, load<int16_t>(c->values, i)); return;
  case FURY_TYPE_INT32: case FURY_TYPE_DATE32: w->Write(ord, load<int32_t>(c->values, i)); return;
  case FURY_TYPE_INT64: case FURY_TYPE_TIMESTAMP: w->Write(ord, load<int64_t>(c->values, i)); return;
  case FURY_TYPE_FLOAT32: w->Write(ord, load<float>(c->values, i)); return;
  case FURY_TYPE_FLOAT64: w->Write(ord, load<double>(c->values, i)); return;
  case FURY_TYPE_STRING: {
    const char *p = static_cast<const char *>(c->values) + c->offsets[i];
    w->WriteString(ord, std::string_view(p, static_cast<size_t>(c->offsets[i + 1] - c->offsets[i])));
    return;
  }
  case FURY_TYPE_BINARY:
    w->WriteBytes(ord, static_cast<const uint8_t *>(c->values) + c->offsets[i],
                  static_cast<uint32_t>(c->offsets[i + 1] - c->offsets[i]));
    return;
  case FURY_TYPE_STRUCT: {
    uint32_t offset = w->cursor();
    nd.row->Reset();
    for (int k = 0; k < f.num_children; k++) {
      write_value(nd.row.get(), false, k, nd.kids[k], &c->child[k], i);
    }
    w->SetOffsetAndSize(ord, offset, w->cursor() - offset);
    return;
  }
  case FURY_TYPE_LIST: {
    uint32_t offset = w->cursor();
    write_array(nd.arr.get(), nd.kids[0], &c->child[0], c->offsets[i], c->offsets[i + 1]);
    w->SetOffsetAndSize(ord, offset, w->cursor() - offset);
    return;
  }
  default: { // MAP
    uint32_t offset = w->cursor();
    w->WriteDirectly(-1);
    write_array(nd.arr.get(), nd.kids[0], &c->child[0], c->offsets[i], c->offsets[i + 1]);
    w->WriteDirectly(offset, static_cast<int64_t>(nd.arr->size()));
    write_array(nd.varr.get(), nd.kids[1], &c->child[1], c->offsets[i], c->offsets[i + 1]);
    w->SetOffsetAndSize(ord, offset, w->cursor() - offset);
    return;
  }
  }
}

// ---- decode ------------------------------------------------------------------------------
// Entries are appended in order, so a node's next free position is always the offset written for
// the previous entry: offsets[idx] (offsets[0] = 0 in a fresh column).
void set_valid(fury_column *c, int64_t idx, bool valid) {
  if (!c->validity) return;
  if (valid) c->validity[idx >> 3] |= static_cast<uint8_t>(1u << (idx & 7));
  else c->validity[idx >> 3] &= static_cast<uint8_t>(~(1u << (idx & 7)));
}

void set_bit(void *bits, int64_t idx, bool on) {
  uint8_t *b = static_cast<uint8_t *>(bits);
  if (on) b[idx >> 3] |= static_cast<uint8_t>(1u << (idx & 7));
  else b[idx >> 3] &= static_cast<uint8_t>(~(1u << (idx & 7)));
}

template <typename T> void store(void *base, int64_t i, T v) {
  std::memcpy(static_cast<uint8_t *>(base) + i * static_cast<int64_t>(sizeof(T)), &v, sizeof(T));
}

void null_entry(const fury_field &f, fury_column *c, int64_t idx) {
  set_valid(c, idx, false);
  switch (f.type_id) {
  case FURY_TYPE_BOOL: set_bit(c->values, idx, false); return;
  case FURY_TYPE_INT8: store<int8_t>(c->values, idx, 0); return;
  case FURY_TYPE_INT16: store<int16_t>(c->values, idx, 0); return;
  case FURY_TYPE_INT32: case FURY_TYPE_DATE32: case FURY_TYPE_FLOAT32:
    store<int32_t>(c->values, idx, 0);
    return;
  case FURY_TYPE_INT64: case FURY_TYPE_TIMESTAMP: case FURY_TYPE_FLOAT64:
    store<int64_t>(c->values, idx, 0);
    return;
  case FURY_TYPE_STRUCT:
    for (int k = 0; k < f.num_children; k++) null_entry(f.children[k], &c->child[k], idx);
    return;
  default: // STRING / BINARY / LIST / MAP: a zero-length entry
    c->offsets[idx + 1] = c->offsets[idx];
    return;
  }
}

void read_value(const fury::Getter &g, int ord, const fury_field &f, fury_column *c, int64_t idx);

void read_array(const fury::ArrayData &a, const fury_field &elem, fury_column *child, int64_t at) {
  for (int j = 0; j < a.num_elements(); j++) read_value(a, j, elem, child, at + j);
}

void read_value(const fury::Getter &g, int ord, const fury_field &f, fury_column *c, int64_t idx) {
  if (g.IsNullAt(ord)) {
    null_entry(f, c, idx);
    return;
  }
  set_valid(c, idx, true);
  switch (f.type_id) {
  case FURY_TYPE_BOOL: set_bit(c->values, idx, g.GetBoolean(ord)); return;
  case FURY_TYPE_INT8: store<int8_t>(c->values, idx, g.GetInt8(ord)); return;
  case FURY_TYPE_INT16: store<int16_t>(c->values, idx, g.GetInt16(ord)); return;
  case FURY_TYPE_INT32: case FURY_TYPE_DATE32: store<int32_t>(c->values, idx, g.GetInt32(ord)); return;
  case FURY_TYPE_INT64: case FURY_TYPE_TIMESTAMP:
    store<int64_t>(c->values, idx, g.GetInt64(ord));
    return;
  case FURY_TYPE_FLOAT32: store<float>(c->values, idx, g.GetFloat(ord)); return;
  case FURY_TYPE_FLOAT64: store<double>(c->values, idx, g.GetDouble(ord)); return;
  case FURY_TYPE_STRING: {
    std::string s = g.GetString(ord);
    int32_t at = c->offsets[idx];
    std::memcpy(static_cast<uint8_t *>(c->values) + at, s.data(), s.size());
    c->offsets[idx + 1] = at + static_cast<int32_t>(s.size());
    return;
  }
  case FURY_TYPE_BINARY: {
    uint8_t *p = nullptr;
    int size = g.GetBinary(ord, &p);
    int32_t at = c->offsets[idx];
    std::memcpy(static_cast<uint8_t *>(c->values) + at, p, static_cast<size_t>(size));
    c->offsets[idx + 1] = at + size;
    return;
  }
  case FURY_TYPE_STRUCT: {
    auto type = std::dynamic_pointer_cast<arrow::StructType>(arrow_type(f));
    std::shared_ptr<fury::Row> row = g.GetStruct(ord, type);
    for (int k = 0; k < f.num_children; k++) read_value(*row, k, f.children[k], &c->child[k], idx);
    return;
  }
  case FURY_TYPE_LIST: {
    std::shared_ptr<fury::ArrayData> a = g.GetArray(ord, fury::list(element_type(f.children[0])));
    int32_t at = c->offsets[idx];
    read_array(*a, f.children[0], &c->child[0], at);
    c->offsets[idx + 1] = at + a->num_elements();
    return;
  }
  default: { // MAP
    auto type = std::dynamic_pointer_cast<arrow::MapType>(arrow_type(f));
    std::shared_ptr<fury::MapData> m = g.GetMap(ord, type);
    int32_t at = c->offsets[idx];
    read_array(*m->keys_array(), f.children[0], &c->child[0], at);
    read_array(*m->values_array(), f.children[1], &c->child[1], at);
    c->offsets[idx + 1] = at + m->num_elements();
    return;
  }
  }
}

bool all_supported(const fury_field *fields, int32_t nfields) {
  for (int k = 0; k < nfields; k++) {
    if (!supported(fields[k])) return false;
  }
  return true;
}

} // namespace

extern "C" {

// Writes nrows rows back to back into out[0, cap) (out == NULL: sizes only) and the exclusive scan
// of their sizes into out_offsets[0 .. nrows].  Returns the total bytes, or -fury_status.
int64_t ref_encode(const fury_field *fields, int32_t nfields, const fury_column *columns,
                   int64_t nrows, uint8_t *out, int64_t cap, int64_t *out_offsets) {
  if (!all_supported(fields, nfields)) return kErrUnsupported;
  auto schema = arrow::schema(arrow_fields(fields, nfields));
  fury::RowWriter top(schema);
  std::vector<Node> nodes(static_cast<size_t>(nfields));
  for (int k = 0; k < nfields; k++) build_node(nodes[k], fields[k], &top);
  int64_t pos = 0;
  for (int64_t i = 0; i < nrows; i++) {
    std::shared_ptr<fury::Buffer> buffer;      // a buffer per row, as RowEncoder.toRow takes one
    fury::AllocateBuffer(64, &buffer);
    top.SetBuffer(buffer);
    top.Reset();
    for (int k = 0; k < nfields; k++) write_value(&top, false, k, nodes[k], &columns[k], i);
    int64_t size = top.size();
    out_offsets[i] = pos;
    if (out) {
      if (pos + size > cap) return kErrCapacity;
      std::memcpy(out + pos, buffer->data() + top.starting_offset(), static_cast<size_t>(size));
    }
    pos += size;
  }
  out_offsets[nrows] = pos;
  return pos;
}

// Fills zero-initialised Arrow-style columns (offsets[0] = 0 everywhere, payload and child buffers
// large enough) from rows the format's writer made.  Valid input only: the reference's getters have
// no bounds rule worth restating.
int ref_decode(const fury_field *fields, int32_t nfields, const uint8_t *rows,
               const int64_t *offsets, int64_t nrows, fury_column *columns) {
  if (!all_supported(fields, nfields)) return FURY_ERR_UNSUPPORTED;
  auto schema = arrow::schema(arrow_fields(fields, nfields));
  auto buffer = std::make_shared<fury::Buffer>(const_cast<uint8_t *>(rows),
                                               static_cast<uint32_t>(offsets[nrows]), false);
  fury::Row row(schema);
  for (int64_t i = 0; i < nrows; i++) {
    row.PointTo(buffer, static_cast<int>(offsets[i]), static_cast<int>(offsets[i + 1] - offsets[i]));
    for (int k = 0; k < nfields; k++) read_value(row, k, fields[k], &columns[k], i);
  }
  return FURY_OK;
}

// Row::ToString of the row at rows[offset, offset + size); returns its length (the text is
// truncated to cap - 1 characters and NUL-terminated), or -fury_status.
int64_t ref_row_to_string(const fury_field *fields, int32_t nfields, const uint8_t *rows,
                          int64_t offset, int64_t size, char *out, int64_t cap) {
  if (!all_supported(fields, nfields)) return kErrUnsupported;
  auto buffer = std::make_shared<fury::Buffer>(const_cast<uint8_t *>(rows),
                                               static_cast<uint32_t>(offset + size), false);
  fury::Row row(arrow::schema(arrow_fields(fields, nfields)));
  row.PointTo(buffer, static_cast<int>(offset), static_cast<int>(size));
  std::string s = row.ToString();
  if (out && cap > 0) {
    size_t n = s.size() < static_cast<size_t>(cap - 1) ? s.size() : static_cast<size_t>(cap - 1);
    std::memcpy(out, s.data(), n);
    out[n] = '\0';
  }
  return static_cast<int64_t>(s.size());
}

} // extern "C"
