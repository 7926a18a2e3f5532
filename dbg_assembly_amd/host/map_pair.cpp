// map_pair -- the link_scaffold module's read-pair mapper (link_scaffold/map_pair.cpp) with every mate mapped on the GPU
// (MAP section of include/dbgk.h).  Same command line, same output files: per pair of reads files
// <name of the first>.map_pair.2ctg.gz, .1ctg.gz, .gap.gz and .stat in -o, and <lib>.map_pair.2ctg.lib beside the library
// file, identical to the reference's after decompression.
#include <ctime>

#include "map_common.h"

static void usage()
{
	cout << "\nFunction instruction:\n\nmap_pair aligns pair of reads to the contigs or scafftigs, using a seed-and-extension globle alignment method. Note that the cutoff for contig size (MinCtgLen -l) is not critical, because link_scaffold will automatically determine the filtering cutoff of small contigs by the insert size of pair-end or mate-paired reads. It is OK to use all or the major part of the contigs for mapping. The recommeded settings is: MinCtgLen (-l) = 1/2 * MinReadLen (-r)\n";
	cout << "\nmap_pair  <contig_file.fa>  <reads_files.lib>\n"
	     << "   Function:  map pair-end or mate-pair reads onto contigs" << endl
	     << "   Version: 1.0" << endl
	     << "   -k <int>     kmer size (construct hash), default=" << KmerSize << endl
	     << "   -s <int>     seed size (number of contained kmers in a seed), default=" << SeedKmerNum << endl
	     << "   -l <int>     contigs not shorter than this cutoff are used for mapping [and scaffolding], default=" << MinCtgLen << endl
	     << "   -r <int>     reads not shorter than this cutoff are used for mapping [and scaffolding], default=" << MinReadLen << endl
	     << "   -i <float>   minimum mapping identity, default=" << MinMapIdentity << endl
	     << "   -f <int>     input file format: 1: fq|gz(one-line), 2: fa|gz(one-line), default=" << Input_file_format << endl
	     << "   -o <str>     output directory, default = " << Output_prefix << endl
	     << "   -h           get the help information\n" << endl
	     << "Example: map_pair  -l 125 -r 250 -o ./maping_results/  Ecoli.contig.fa illumina_reads.lib" << endl
	     << endl;
	exit(0);
}

// the counters of one pair of reads files
struct PairTally {
	uint64_t total_read_pair_num = 0, map_ctg_diff_num = 0, map_ctg_same_num = 0, map_ctg_gap_num = 0, map_no_no_num = 0;
	void write(ofstream &MapCtgStat) const
	{
		MapCtgStat << "\ttotal_read_pair_num: " << total_read_pair_num << endl;
		MapCtgStat << "\tmap_ctg_diff_num: " << map_ctg_diff_num << "  " << (double)map_ctg_diff_num / total_read_pair_num * 100 << "%" << endl;
		MapCtgStat << "\tmap_ctg_same_num: " << map_ctg_same_num << "  " << (double)map_ctg_same_num / total_read_pair_num * 100 << "%" << endl;
		MapCtgStat << "\tmap_ctg_gap_num: " << map_ctg_gap_num << "  " << (double)map_ctg_gap_num / total_read_pair_num * 100 << "%" << endl;
		MapCtgStat << "\tmap_no_no_num: " << map_no_no_num << "  " << (double)map_no_no_num / total_read_pair_num * 100 << "%" << endl;
	}
};

// one pair with the first hit of each mate -> its line in one of the three files (the body of the loop of map_pair.cpp:284-340)
static void rows_of_pair(const Contigs &ctg, const string &id1, size_t len, const dbgk_map_hit &a, const string &id2, size_t len2, const dbgk_map_hit &b,
                         PairTally &T, ostringstream &diff, ostringstream &same, ostringstream &gap)
{
	T.total_read_pair_num++;
	if (a.contig != -1 && b.contig != -1) {
		ostringstream &o = a.contig != b.contig ? diff : same;
		(a.contig != b.contig ? T.map_ctg_diff_num : T.map_ctg_same_num)++;
		ctg.row(o, id1, len, a);
		o << "\t";
		ctg.row(o, id2, len2, b);
		o << "\n";
	} else if (a.contig != -1 || b.contig != -1) {
		T.map_ctg_gap_num++;
		if (a.contig != -1) {
			ctg.row(gap, id1, len, a);
			gap << "\n";
		}
		if (b.contig != -1) {
			ctg.row(gap, id2, len2, b);
			gap << "\n";
		}
	} else {
		T.map_no_no_num++;
	}
}

static const char *read_id_delims() { return Input_file_format == 1 ? "@ \t" : "> \t"; } // make_read_id of map_pair.cpp:222

// one pair of reads files (parse_two_paired_reads_file, map_pair.cpp:152-354)
static void parse_two_paired_reads_file(const Contigs &ctg, const string &input_reads_file, const string &input2_reads_file)
{
	LineReader infile(input_reads_file), infile2(input2_reads_file);
	const string name = Output_prefix + "/" + base_name(input_reads_file);
	GzWriter MapCtgDiff(name + ".map_pair.2ctg.gz"), MapCtgSame(name + ".map_pair.1ctg.gz"), MapCtgGap(name + ".map_pair.gap.gz");
	const string stat_file = name + ".map_pair.stat";
	ofstream MapCtgStat(stat_file.c_str());
	if (!MapCtgStat) cerr << "fail to open output file " << stat_file << endl;
	MapCtgDiff.write(string(HeaderOne) + HeaderTwo + "\n");
	MapCtgSame.write(string(HeaderOne) + "\n");
	MapCtgGap.write(string(HeaderOne) + "\n");

	PairTally T;
	ReadBatch batch; // mates side by side: read 2i and 2i + 1 are pair i
	vector<string> ids;

	auto flush = [&]() {
		batch.map(ctg.mapper);
		ostringstream diff, same, gap;
		for (size_t i = 0; i + 1 < batch.size(); i += 2) {
			const size_t len = batch.offsets[i + 1] - batch.offsets[i], len2 = batch.offsets[i + 2] - batch.offsets[i + 1];
			rows_of_pair(ctg, ids[i], len, batch.hits[2 * i], ids[i + 1], len2, batch.hits[2 * (i + 1)], T, diff, same, gap);
		}
		MapCtgDiff.write(diff.str());
		MapCtgSame.write(same.str());
		MapCtgGap.write(gap.str());
		batch.clear();
		ids.clear();
	};

	// the record loop of map_pair.cpp:213-272: every line the loop takes from the first file is one round; a line that is no
	// header leaves the previous pair in place, which is then mapped and counted again
	string read, read_head, read_id, read2, read2_head, read2_id, line_no_use;
	const char mark = Input_file_format == 1 ? '@' : '>';
	const char *delim = read_id_delims();
	while (infile.getline(read_head)) {
		if ((Input_file_format == 1 || Input_file_format == 2) && !read_head.empty() && read_head[0] == mark) {
			read_id = make_read_id(read_head, delim);
			infile.getline(read);
			if (Input_file_format == 1) {
				infile.getline(line_no_use);
				infile.getline(line_no_use);
			}
			infile2.getline(read2_head);
			read2_id = make_read_id(read2_head, delim);
			infile2.getline(read2);
			if (Input_file_format == 1) {
				infile2.getline(line_no_use);
				infile2.getline(line_no_use);
			}
		}
		if (read.size() < (size_t)MinReadLen || read2.size() < (size_t)MinReadLen) continue;
		ids.push_back(read_id);
		ids.push_back(read2_id);
		batch.add(read);
		batch.add(read2);
		if (batch.full()) flush();
	}
	flush();
	MapCtgDiff.close();
	MapCtgSame.close();
	MapCtgGap.close();
	T.write(MapCtgStat);
}

// what the device batch cannot reproduce: the program ends with status 1 (clean_adapter set the precedent)
[[noreturn]] static void refuse_on_device(const string &what)
{
	cerr << what << ": DBGK_TEXT=device cannot reproduce this, run without it" << endl;
	exit(1);
}

// DBGK_TEXT=device: parse_two_paired_reads_file on the route where the text of the files never becomes strings.  A window of each
// file is parsed (ParsedFile of map_common.h); read i of the first batch and read i of the second are pair i.  When the two windows
// deliver different numbers of records, the first min(n1, n2) of both are taken and the longer one hands its surplus back to its
// window loop from the header of record n on.  Each mate's batch goes through the one mapper, its hits are taken over as a side of
// the row writer, and dbgk_maprow_rows_device classifies the pairs and composes the lines of the three files, which leave through
// GzWriter::write_device.  Refused, because the loop above does something with them that a batch of records cannot express: a line
// in front of a header in either file (the loop maps the previous pair again on such a line of the first file, and takes any line
// of the second as a header), and files that do not hold the same number of records.
static void parse_two_paired_reads_file_on_device(const Contigs &ctg, const string &input_reads_file, const string &input2_reads_file)
{
	const string name = Output_prefix + "/" + base_name(input_reads_file);
	GzWriter MapCtgDiff(name + ".map_pair.2ctg.gz"), MapCtgSame(name + ".map_pair.1ctg.gz"), MapCtgGap(name + ".map_pair.gap.gz");
	GzWriter *const out[DBGK_MAPROW_STREAMS] = {&MapCtgDiff, &MapCtgSame, &MapCtgGap};
	const string stat_file = name + ".map_pair.stat";
	ofstream MapCtgStat(stat_file.c_str());
	if (!MapCtgStat) cerr << "fail to open output file " << stat_file << endl;
	MapCtgDiff.write(string(HeaderOne) + HeaderTwo + "\n");
	MapCtgSame.write(string(HeaderOne) + "\n");
	MapCtgGap.write(string(HeaderOne) + "\n");

	PairTally T;
	ParsedFile f1(input_reads_file), f2(input2_reads_file);
	ParsedFile *const file[2] = {&f1, &f2};
	const string *const path[2] = {&input_reads_file, &input2_reads_file};
	uint64_t records = 0, out_bytes = 0, host_batches = 0;
	double ms_map = 0, ms_rows = 0;
	for (;;) {
		const bool more[2] = {f1.next(), f2.next()};
		if (!more[0] && !more[1]) break;
		for (int k = 0; k < 2; k++)
			if (more[k] && file[k]->pi.ignored_lines)
				refuse_on_device(to_string(file[k]->pi.ignored_lines) + " line(s) of " + *path[k] + " stand in front of a header");
		for (int k = 0; k < 2; k++)
			if (!more[k] && file[1 - k]->pi.n_records) refuse_on_device(*path[0] + " and " + *path[1] + " do not hold the same number of records");
		const uint64_t n = more[0] && more[1] ? min(f1.pi.n_records, f2.pi.n_records) : 0;
		if (n) {
			records += n;
			dbgk_maprow_side sides[2];
			for (int k = 0; k < 2; k++) {
				file[k]->map_into(ctg, k, n);
				dbgk_map_stats ms;
				const int rc = dbgk_map_batch_stats(ctg.mapper, &ms);
				if (rc) die("dbgk_map_batch_stats", rc);
				ms_map += ms.ms_map + ms.ms_long;
				sides[k] = file[k]->side;
			}
			dbgk_maprow_info ri;
			const int rc = dbgk_maprow_rows_device(ctg.rows, sides, n, &ri);
			if (rc) die("dbgk_maprow_rows_device", rc);
			ms_rows += ri.ms_scan + ri.ms_write;
			if (ri.unprintable || rows_forced_to_host()) {
				vector<string> heads[2];
				string bases[2];
				vector<uint64_t> offsets[2];
				vector<dbgk_map_hit> hits[2];
				for (int k = 0; k < 2; k++) file[k]->to_host(ctg, n, heads[k], bases[k], offsets[k], hits[k]);
				ostringstream diff, same, gap;
				for (uint64_t i = 0; i < n; i++) {
					const size_t len = offsets[0][i + 1] - offsets[0][i], len2 = offsets[1][i + 1] - offsets[1][i];
					if (len < (size_t)MinReadLen || len2 < (size_t)MinReadLen) continue;
					rows_of_pair(ctg, make_read_id(heads[0][i], read_id_delims()), len, hits[0][2 * i], make_read_id(heads[1][i], read_id_delims()), len2,
					             hits[1][2 * i], T, diff, same, gap);
				}
				MapCtgDiff.write(diff.str());
				MapCtgSame.write(same.str());
				MapCtgGap.write(gap.str());
				host_batches++;
			} else {
				T.total_read_pair_num += ri.counters[0], T.map_ctg_diff_num += ri.counters[1], T.map_ctg_same_num += ri.counters[2];
				T.map_ctg_gap_num += ri.counters[3], T.map_no_no_num += ri.counters[4];
				for (int s = 0; s < DBGK_MAPROW_STREAMS; s++) {
					out[s]->write_device(ctg.rows, s);
					out_bytes += ri.stream_bytes[s];
				}
			}
		}
		for (int k = 0; k < 2; k++) {
			if (!more[k]) continue;
			ParsedFile &F = *file[k];
			if (F.pi.n_records > n) { // the surplus goes back: the next text begins with the header of record n
				dbgk_parse_rec at;
				vector<dbgk_parse_rec> recs(F.pi.n_records);
				const int rc = dbgk_parse_results(F.parser, nullptr, nullptr, nullptr, recs.data());
				if (rc) die("dbgk_parse_results", rc);
				at = recs[n];
				F.in.keep_from(at.head_pos, true);
			} else {
				F.in.keep_from(F.pi.consumed);
			}
		}
	}
	MapCtgDiff.close();
	MapCtgSame.close();
	MapCtgGap.close();
	if (getenv("DBGK_TIMINGS"))
		cerr << "Text on device: " << f1.in.windows << " windows, " << records << " records, " << out_bytes << " bytes of rows, " << host_batches
		     << " batches through the host loop; device ms: parse " << f1.ms_parse + f2.ms_parse << ", map " << ms_map << ", rows " << ms_rows << endl;
	T.write(MapCtgStat);
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "k:s:l:r:i:f:o:h")) != -1) {
		switch (c) {
			case 'k': KmerSize = atoi(optarg); break;
			case 's': SeedKmerNum = atoi(optarg); break;
			case 'l': MinCtgLen = atoi(optarg); break;
			case 'r': MinReadLen = atoi(optarg); break;
			case 'i': MinMapIdentity = atof(optarg); break;
			case 'f': Input_file_format = atoi(optarg); break;
			case 'o': Output_prefix = optarg; break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 3 || argc - optind < 2) usage();
	const string contig_seq_file = argv[optind++];
	const string reads_lib_file = argv[optind++];

	const clock_t time_start = clock();
	cerr << "\nProgram start ............" << endl;
	vector<string> reads_files;
	reading_lib_file(reads_lib_file, reads_files);
	cerr << "\nInput reads file number: " << reads_files.size() << endl;
	for (const string &f : reads_files) cerr << f << endl;
	if (reads_files.size() % 2) {
		cerr << "map_pair: the library file lists an odd number of reads files" << endl;
		return 1;
	}

	{
		const string mapped_2ctg_file = reads_lib_file + ".map_pair.2ctg.lib";
		ofstream TwoCtgFile(mapped_2ctg_file.c_str());
		for (size_t i = 0; i < reads_files.size(); i += 2) TwoCtgFile << Output_prefix << "/" << reads_files[i] << ".map_pair.2ctg.gz" << endl;
	}

	Contigs ctg;
	ctg.load(contig_seq_file, 0);
	const bool on_device = text_on_device();
	if (on_device) ctg.rows_on_device(DBGK_MAPROW_PAIR, read_id_delims());
	make_output_dir();

	cerr << "\nparse input reads files: " << endl;
	for (size_t i = 0; i < reads_files.size(); i += 2) {
		cerr << "\n\t" << reads_files[i] << " ............." << endl;
		cerr << "\n\t" << reads_files[i + 1] << " ............." << endl;
		if (on_device) parse_two_paired_reads_file_on_device(ctg, reads_files[i], reads_files[i + 1]);
		else parse_two_paired_reads_file(ctg, reads_files[i], reads_files[i + 1]);
	}
	cerr << "\nProgram finished !" << endl;
	cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl;
	return 0;
}
